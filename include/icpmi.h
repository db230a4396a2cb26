/*
 * include/icpmi.h -- C ABI of the MI355X-native ICP registration core ("icpmi").
 *
 * This is the drop-in boundary for the hot path of norlab_icp_mapper (reference tree
 * /root/reference, v2.1.0).  The reference has no FFI of its own: the path is entered through the
 * in-process C++ object `PM::ICPSequence icp` (norlab_icp_mapper/Mapper.h:23) and the MapperModule
 * virtuals (norlab_icp_mapper/MapperModules/MapperModule.h:20-29).  Each entry point below names the
 * reference interface it replaces; INTEGRATION.md shows the C++ shim (`GpuICPSequence`,
 * `Gpu*MapperModule`) a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C, no torch / Eigen / HIP types in any signature;
 *   - clouds are `features` blocks of PM::DataPoints: 4 x N column-major float (x,y,z,1), i.e. N
 *     consecutive float4; normals are 3 x N column-major float (descriptor "normals");
 *   - 4x4 transforms are column-major float[16] (Eigen's default, PM::TransformationParameters);
 *   - pointers are HOST pointers unless the function name ends in `_dev`, in which case cloud
 *     pointers are device (HBM) pointers on the handle's GPU; the callee never retains caller
 *     memory (DataPoints value semantics, SURVEY.md 8b "Ownership");
 *   - every function returns an icpmi_status; icpmi_last_error(h) gives the message.  The reference
 *     reports the same conditions as C++ exceptions (PM::ConvergenceError, ...); the mapping is
 *     given next to each status code;
 *   - one HIP stream per handle; every entry point locks its handle for the duration of the call, so
 *     calls on one handle from several threads are safe and run one after the other (the reference
 *     serialises icp() and icp.setMap() with icpMapLock, Mapper.cpp:212, Map.cpp:527-529, but its
 *     modules and filters -- each with a private kd-tree -- run outside that lock: online mode reaches
 *     one handle from the caller's thread, the std::async update thread and the paging thread);
 *     pairs of calls that hand state to each other (icpmi_register_prior -> icpmi_map_update_*_staged)
 *     still belong to one logical owner; different handles are independent (one per GPU).
 */
#ifndef ICPMI_H
#define ICPMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICPMI_VERSION 4

typedef struct icpmi_ctx* icpmi_handle;

typedef enum {
    ICPMI_OK = 0,
    ICPMI_ERR_INVALID_ARG = 1,          /* PM::Parametrizable::InvalidParameter / std::invalid_argument */
    ICPMI_ERR_HIP = 2,                  /* device runtime failure (no reference analogue)               */
    ICPMI_ERR_NO_POINT_TO_MINIMIZE = 3, /* PM::ConvergenceError("ErrorMnimizer: no point to minimize")  */
    ICPMI_ERR_NO_OUTLIER_TO_FILTER = 4, /* PM::ConvergenceError("no outlier to filter")                 */
    ICPMI_ERR_BOUND = 5,                /* PM::ConvergenceError from BoundTransformationChecker         */
    ICPMI_ERR_NAN = 6,                  /* PM::ConvergenceError("abs rotation norm not a number")       */
    ICPMI_ERR_MISSING_NORMALS = 7,      /* PM::DataPoints::InvalidField("normals")                      */
    ICPMI_ERR_UNSUPPORTED = 8
} icpmi_status;

/* ErrorMinimizer selection (icp.errorMinimizer in the YAML chain, Mapper.cpp:72) */
typedef enum {
    ICPMI_MIN_IDENTITY = 0,       /* IdentityErrorMinimizer (examples/config.yaml:62-63) */
    ICPMI_MIN_POINT_TO_POINT = 1, /* PointToPointErrorMinimizer                          */
    ICPMI_MIN_POINT_TO_PLANE = 2, /* PointToPlaneErrorMinimizer (docs/MapperConfiguration.md:174-189) */
    /* PlaneToPlaneErrorMinimizer{epsilon, force4DOF}: generalized ICP (Segal, Haehnel, Thrun 2009) with plane-regularised covariances
     * from the normals of BOTH clouds -- not libpointmatcher's.  Per pair, p = T_iter x, q its match, n_q the match's normal, n_p = R n_x
     * the reading point's normal under T_iter's rotation (each normalised; a zero or non-finite normal: that side's covariance is I):
     *     C(n) = I - (1 - eps) n n^T,  M = (C(n_q) + C(n_p))^-1 (adjugate / determinant, float),  J = [-[p]x  I],  d = p - q
     *     A += w J^T M J,  b -= w J^T M d      (x = (omega, t); with M = n n^T this IS the point-to-plane system)
     * M is re-formed every iteration from the current rotation and held during the solve.  The sums fill the point-to-plane slots
     * (icpmi_minimize_step_normals: sums[0..20] A, [21..26] b, [27] sum w, [28] pairs) and the point-to-plane solve runs on them, force4DOF
     * included.  eps: icpmi_set_plane_epsilon (default 1e-3).  The map AND the reading must carry normals: the entry points that take
     * scan_normals3 serve it (icpmi_register, _dev, _fixed_dev, icpmi_minimize_step_normals) and return ICPMI_ERR_MISSING_NORMALS when the
     * map has none or scan_normals3 is NULL -- as icpmi_register_prior* do, which carry none; icpmi_register_batch_dev,
     * icpmi_register_multistart* and icpmi_minimize_step cannot carry them: ICPMI_ERR_UNSUPPORTED.  Rejected with ICPMI_ERR_INVALID_ARG:
     * force_2d / is_2d, covariance = 1 (Censi's form is derived for the scalar residual), degeneracy_threshold != 0 (mu = lambda / sum w
     * assumes unit-information pairs; M's scale is 1 / (2 eps)).  icpmi_residual_error* on such a handle reports the point-to-plane
     * residual |(p - q) . n_q| (ICPMI_RES_CHAIN = ICPMI_RES_POINT_TO_PLANE); the sensor-noise overlap is the point-to-plane count.
     * This is the pair model ICPMI_PLANE_MODEL_GICP, the default; icpmi_set_plane_pair_model puts the symmetric point-to-plane model
     * (ICPMI_PLANE_MODEL_SYMMETRIC, below) on the same path. */
    ICPMI_MIN_PLANE_TO_PLANE = 3
} icpmi_minimizer;

/* OutlierFilters (icp.outlierFilters) */
typedef enum {
    ICPMI_OUT_MAXDIST = 1,      /* MaxDistOutlierFilter{maxDist}        w = d2 <= maxDist^2          */
    ICPMI_OUT_MINDIST = 2,      /* MinDistOutlierFilter{minDist}        w = d2 >= minDist^2          */
    ICPMI_OUT_MEDIANDIST = 3,   /* MedianDistOutlierFilter{factor}      w = d2 <= factor*median(d2)  */
    ICPMI_OUT_TRIMMEDDIST = 4,  /* TrimmedDistOutlierFilter{ratio}      w = d2 <= quantile(d2,ratio) */
    ICPMI_OUT_SURFACENORMAL = 5,/* SurfaceNormalOutlierFilter{maxAngle} w = n_read.n_ref > cos(maxAngle) */
    /* GenericDescriptorOutlierFilter{source: reference, descName, useSoftThreshold, useLargerThan, threshold}: the 1-row descriptor
     * of the matched map point -- the tracked scalar channel, icpmi_set_map_scalar -- decides.  param = threshold, iparam = flags.
     * hard: w = desc > threshold (useLargerThan) or desc < threshold; soft: w = desc.  source: reading (iparam | ICPMI_GEN_SOURCE_READING,
     * v4): the descriptor of the READING point decides -- its row is handed over with icpmi_set_reading_scalar before every registration. */
    ICPMI_OUT_GENERICDESCRIPTOR = 6,
    /* RobustOutlierFilter{robustFct, tuning, scaleEstimator: none | mad | berg | std, nbIterationForScale, distanceType,
     * approximation}: M-estimator weight of e2 = residual / scale^2.  param = tuning, param2 = nbIterationForScale, param3 =
     * approximation (0 or +inf: none; e2 >= approximation^2 forces the weight to 0), iparam = robustFct | scaleEstimator << 4 |
     * distanceType << 8.  berg (r5): scale 1.9 sqrt(median d2) at iteration 1, then 0.85 (scale - tuning) + tuning, with Bergstrom's
     * constants as the M-estimator's tuning (cauchy 4.3040, tukey 7.0589, huber 2.0138).  std (r5): sqrt of the standard deviation of
     * EVERY entry of the distance matrix (an infinite entry makes the registration end with ICPMI_ERR_NAN, as it poisons upstream's). */
    ICPMI_OUT_ROBUST = 7,
    /* VarTrimmedDistOutlierFilter{minRatio, maxRatio, lambda} (Phillips et al. 2007): TrimmedDist at the ratio that minimises
     * FRMS(i) = (sum of the i + 1 smallest d2) / ((i + 1) ((i + 1) / N)^(2 lambda)) over floor(minRatio N) <= i < floor(maxRatio N).
     * param = minRatio, param2 = maxRatio, param3 = lambda. */
    ICPMI_OUT_VARTRIMMEDDIST = 8
} icpmi_outlier_type;
enum { ICPMI_GEN_SOURCE_READING = 1, ICPMI_GEN_SOFT = 2, ICPMI_GEN_LARGER = 4 };
enum { ICPMI_ROB_CAUCHY = 0, ICPMI_ROB_WELSCH = 1, ICPMI_ROB_SC = 2, ICPMI_ROB_GM = 3, ICPMI_ROB_TUKEY = 4, ICPMI_ROB_HUBER = 5,
       ICPMI_ROB_L1 = 6, ICPMI_ROB_STUDENT = 7 };
enum { ICPMI_SCALE_NONE = 0, ICPMI_SCALE_MAD = 1, ICPMI_SCALE_BERG = 2, ICPMI_SCALE_STD = 3 };
enum { ICPMI_DIST_POINT2POINT = 0, ICPMI_DIST_POINT2PLANE = 1 };

typedef struct {
    int32_t type; /* icpmi_outlier_type */
    float   param;
    int32_t iparam; /* flags / enums of GenericDescriptor and Robust, 0 otherwise */
    float   param2; /* Robust: nbIterationForScale; VarTrimmedDist: maxRatio        */
    float   param3; /* VarTrimmedDist: lambda; Robust: approximation (0 / +inf: none)  */
} icpmi_outlier;

typedef enum { ICPMI_STOP_NONE = 0, ICPMI_STOP_COUNTER = 1, ICPMI_STOP_DIFFERENTIAL = 2 } icpmi_stop_reason;

/* The ICP chain of PM::ICPSequence::loadFromYamlNode (Mapper.cpp:72) restricted to the modules on
 * the hot path.  icpmi_config_default() fills libpointmatcher's defaults for those modules. */
typedef struct {
    int32_t device;            /* HIP device ordinal                                              */
    /* matcher: KDTreeMatcher (KDTreeVarDistMatcher: var_dist below) */
    int32_t knn;               /* default 1                                                       */
    float   max_dist;          /* default +inf; ignored when var_dist = 1                         */
    float   epsilon;           /* default 0; > 0 is served by the EXACT search (a valid epsilon-    */
                               /* answer, but not libnabo's pick -- SURVEY.md 0.4) unless           */
                               /* epsilon_approx below asks for libnabo's pruning                   */
    /* outlier filters, applied in order, weights multiply */
    int32_t n_outlier;
    icpmi_outlier outlier[8];
    /* error minimiser */
    int32_t minimizer;         /* icpmi_minimizer                                                 */
    int32_t force_4dof;        /* PointToPlaneErrorMinimizer.force4DOF: yaw + translation only     */
    int32_t force_2d;          /* PointToPlaneErrorMinimizer.force2D on 3-D clouds: yaw + (tx, ty), */
                               /* residual = the 2-D dot with the top two rows of the normals       */
    int32_t is_2d;             /* planar clouds (the mapper's is3D == false, Mapper.h:53): every    */
                               /* point has z == 0; point-to-point solves the 2-D rotation,         */
                               /* point-to-plane the force2D system, SurfaceNormal the 2 x 2 problem */
    /* transformation checkers */
    int32_t max_iterations;    /* CounterTransformationChecker.maxIterationCount, default 40      */
    int32_t use_differential;  /* DifferentialTransformationChecker present                       */
    float   min_diff_rot;      /* default 0.001                                                   */
    float   min_diff_trans;    /* default 0.001                                                   */
    int32_t smooth_length;     /* default 3 (<= 16)                                               */
    int32_t use_bound;         /* BoundTransformationChecker present                              */
    float   max_rot_norm;      /* default 1                                                       */
    float   max_trans_norm;    /* default 1                                                       */
    /* engine knobs (no reference analogue) */
    float   grid_cell;         /* NN grid cell edge in metres; 0 = choose from the map density     */
    int32_t use_graph;         /* 1 = fixed-iteration registrations replay one hipGraph (default) */
    int32_t profile;           /* 1 = eager launches with HIP events around every NN launch        */
    int32_t fuse_solve;        /* (v4) asked for the solve inside the next NN launch (three launches per iteration).  The path lost  */
                               /* on two of three shapes and was REMOVED in r5: the field keeps the struct's layout    */
                               /* and is ignored (every value runs the four-launch iteration, bit-identical results as before).     */
    /* r6: the two switches of the k > 1 matcher that tests still need were environment variables through r5 (read once per process); they are
       per-handle fields now.  Zero = the default, so a zeroed tail keeps every old caller's behaviour.                                        */
    int32_t knn_wg_from;       /* which iterations of a k > 1 loop nnk_wg_kernel serves: 0 = from iteration 2 (default), n > 0 = from          */
                               /* iteration n - 1, < 0 = none (nnk_ml_kernel everywhere).  Same bits either way (tests/test_gpu_knn_wg.py).    */
    int32_t sel_window_off;    /* 1 = the quantile selection of a k > 1 loop always builds its full level-0 histogram (no speculative window, */
                               /* DESIGN_history.md 13.7b).  Same bits either way (tests/test_gpu_sel_window.py).                              */
    int32_t epsilon_approx;    /* (r6) 1 = `epsilon` prunes the matcher's search as libnabo's maxError2 does (`new_rd * (1 + epsilon)^2 <         */
                               /* heap.headValue()`): cells farther than (k-th distance so far) / (1 + epsilon) are not visited, a query is decided  */
                               /* once its k-th distance is within (1 + epsilon) x the margin of its block.  Every returned distance d_j <=           */
                               /* (1 + epsilon) x the exact j-th distance (tests/test_gpu_epsilon.py); WHICH valid answer comes back differs from     */
                               /* libnabo's (its pick depends on the kd-tree's traversal order).  0 (default): the exact search.  k <= 16; filters'   */
                               /* own searches (PointDistance, SurfaceNormal) stay exact.                                                              */
    int32_t covariance;        /* PointToPlaneWithCovErrorMinimizer: 1 = every single registration leaves the 6 x 6 pose covariance for       */
                               /* icpmi_get_covariance (two launches after the loop); point-to-plane on 3-D clouds only.  Default 0.          */
    float   sensor_std_dev;    /* PointToPlaneWithCovErrorMinimizer.sensorStdDev: sigma of the range noise, finite and >= 0, default 0.01    */
    union {                    /* var_dist IS reserved[0]: a caller compiled before the field existed zeroes it with the rest of the tail         */
        int32_t var_dist;      /* 1 = the matcher is KDTreeVarDistMatcher{knn, epsilon, maxDistField}: reading point i is matched within ITS OWN   */
                               /* radius, entry i of the row icpmi_set_reading_max_dist hands over before every registration; max_dist is        */
                               /* ignored.  0 (default): KDTreeMatcher, every result as before the field existed.                                 */
        struct {               /* degeneracy_threshold IS reserved[1], the same way                                                                */
            int32_t var_dist_;
            float degeneracy_threshold; /* degeneracy-aware point-to-plane minimiser (icpmi_get_localizability): 0 (default) = off, every result  */
                               /* as before the field existed; t > 0 = solve every iteration only in the span of the directions whose normalised   */
                               /* information mu exceeds t, and report; t < 0 = report only, flags against |t|, poses bit-identical to 0.  Finite;  */
                               /* point-to-plane on 3-D clouds only (no force_2d / is_2d).                                                         */
        };
        int32_t reserved[2];
    };
} icpmi_config;

/* What PM::ICPSequence exposes after a call: errorMinimizer->getOverlap() (Mapper.cpp:219) is
 * weighted_point_used_ratio; the inspector statistics of SURVEY.md section 5 are the rest. */
typedef struct {
    int32_t iterations;
    int32_t stop_reason;               /* icpmi_stop_reason                                       */
    int64_t pairs;                     /* P of the last iteration                                 */
    float   point_used_ratio;          /* P / (knn N)                                             */
    float   weighted_point_used_ratio; /* sum w / (knn N) == getOverlap()                         */
    float   trimmed_limit;             /* last quantile limit on d^2 (Trimmed / Median), else -1  */
    float   loop_ms;                   /* device time of the iteration loop (HIP events)          */
    float   nn_ms_avg;                 /* mean NN launch time: profile mode = HIP events (event-pair gap removed); otherwise device  */
                                       /* clocks from the NN kernel's first workgroup to the first workgroup of the next kernel       */
    int32_t nn_launches;               /* number of NN launches averaged                          */
    int64_t hard_queries;              /* NN queries the grid pyramid could not decide (brute pass) */
    int32_t reserved[4];
    float   sensor_noise_overlap;      /* getOverlap() of a reading that carries `simpleSensorNoise` and `normals`
                                          (icpmi_set_reading_sensor_noise): the share of the last iteration's pairs within the
                                          sensor noise; -1 when not computed (then getOverlap() == weighted_point_used_ratio) */
    int32_t reserved2;
} icpmi_stats;

void icpmi_config_default(icpmi_config* cfg);

/* Replaces constructing / configuring `PM::ICPSequence icp` (Mapper.h:23, Mapper.cpp:72,77). */
icpmi_status icpmi_create(const icpmi_config* cfg, icpmi_handle* out);
/* Re-configure the chain of an existing handle (`icp.loadFromYamlNode` / `icp.setDefault()` called
 * again on the same object): the handle, its device and its map stay. cfg->device must not change. */
icpmi_status icpmi_set_config(icpmi_handle h, const icpmi_config* cfg);
void         icpmi_destroy(icpmi_handle h);
const char*  icpmi_last_error(icpmi_handle h); /* h may be NULL: error of the last failed create */

/* Replaces `bool PM::ICPSequence::setMap(const DataPoints&)` (Map.cpp:111,178,528,581): copies the
 * cloud, centres it on its centroid, builds the NN index on the device.  *accepted = 0 and state
 * unchanged when m == 0 (upstream returns false and warns).  normals3 may be NULL. */
icpmi_status icpmi_set_map(icpmi_handle h, const float* map4, int64_t m, const float* normals3, int32_t* accepted);
icpmi_status icpmi_set_map_dev(icpmi_handle h, const float* d_map4, int64_t m, const float* d_normals3, int32_t* accepted);
/* `icp.hasMap()` */
int32_t      icpmi_has_map(icpmi_handle h);
/* centroid used for centring (T_refIn_refMean translation) */
icpmi_status icpmi_get_map_mean(icpmi_handle h, float mean3[3]);

/* `ErrorMinimizer::getOverlap()` (read at Mapper.cpp:219, used by the `overlap` update condition, Mapper.cpp:257-260): when the reading
 * carries the descriptors `simpleSensorNoise` (1 x N) and `normals`, upstream's minimisers do not return the weighted ratio but the share of
 * the last iteration's pairs that lie within the sensor noise -- PointToPoint: |p - q| < mean|p - q| + noise_i; PointToPlane:
 * |(p - q) . n_i / |n_i|| < noise_i with n_i the READING's normal.  This call hands over the noise row of the NEXT registration's reading
 * (host pointer, n floats, one shot: it is consumed by that registration, whose scan_normals3 must be given and whose n must match; any
 * other case leaves stats.sensor_noise_overlap at -1).  noise == NULL or n == 0 clears it. */
icpmi_status icpmi_set_reading_sensor_noise(icpmi_handle h, const float* noise, int64_t n);

/* (v4) GenericDescriptorOutlierFilter{source: reading}: the 1-row descriptor `descName` of the NEXT registration's reading (host pointer, n
 * floats, one shot: consumed by that registration, whose n must match -- else it fails with InvalidField like upstream's missing descriptor).
 * scalar == NULL or n == 0 clears it.  Registrations of a batch with such a chain are not served (every reading needs its own row). */
icpmi_status icpmi_set_reading_scalar(icpmi_handle h, const float* scalar, int64_t n);

/* KDTreeVarDistMatcher (icpmi_config::var_dist = 1; libpointmatcher's matcher AS RECALLED: upstream's source is not on hand): the 1-row
 * descriptor `maxDistField` (default name `maxSearchDist`) of the NEXT registration's reading -- radii[i] is the search radius of reading
 * point i, a distance; libnabo's `knn(query, ids, dists, maxRadii, k, epsilon, flags)` squares it.  Query i gets its up-to-knn nearest map
 * points with d2 <= radii[i]^2 (the float product, +inf for +inf: the expression that squares KDTreeMatcher's maxDist, so a constant row
 * gives the bits of `maxDist`); the other slots stay unfilled (-1 / +inf).  Same contract as icpmi_set_reading_scalar: host pointer, n floats,
 * one shot -- consumed by the next registration, whose n must match; a registration on a var_dist handle without a row, or with another n,
 * fails with ICPMI_ERR_INVALID_ARG ("InvalidField: ..."), upstream's missing descriptor.  Every entry must be >= 0 or +inf: a NaN or a
 * negative entry is ICPMI_ERR_INVALID_ARG here.  An entry 0 is valid (that point matches nothing but a coincident map point); a row whose
 * LARGEST entry is 0 makes the registration fail with ICPMI_ERR_INVALID_ARG, as `maxDist: 0` does ("must be > 0").  radii == NULL or
 * n == 0 clears the row.  The search itself runs with ONE bound, the largest entry of the row (+inf if any entry is +inf); only the
 * accept test is per query.  icpmi_register_batch_dev on a var_dist handle registers one reading after the other (every reading needs
 * its own row: the rule reading-scalar chains follow); icpmi_minimize_step is not served (ICPMI_ERR_UNSUPPORTED).  Planar handles are
 * served as elsewhere. */
icpmi_status icpmi_set_reading_max_dist(icpmi_handle h, const float* radii, int64_t n);

/* Replaces `TransformationParameters PM::ICPSequence::operator()(const DataPoints&)`
 * (Mapper.cpp:213): scan4 is the reading already moved by the prior (Mapper.cpp:197); T_out is the
 * correction in the map frame (so that correctedPose = T_out * estimatedPose, Mapper.cpp:215).
 * Without a map returns identity and ICPMI_OK like upstream. scan_normals3 may be NULL. */
icpmi_status icpmi_register(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3,
                            float T_out[16], icpmi_stats* stats);
icpmi_status icpmi_register_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3,
                                float T_out[16], icpmi_stats* stats);
/* Throughput mode: run exactly `iterations` loop passes (Counter only) -- what the bench times. */
icpmi_status icpmi_register_fixed_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3,
                                      int32_t iterations, float T_out[16], icpmi_stats* stats);

/* `icp(input)` for `batch` independent readings against the same map in ONE launch sequence (no reference analogue: the
 * reference registers one scan per call, Mapper.cpp:213; this is what a multi-stream front end -- BASELINE config 5: several
 * scan streams against a shared map -- calls instead of `batch` registrations): every kernel of the loop runs once per
 * iteration for all readings (blockIdx.y = reading), each reading keeps its own loop state and stops on its own checkers.
 * Results are bit-identical to registering each reading alone.  d_scans4: host array of `batch` device pointers (readings
 * already moved by their priors), n: their sizes; fixed_iterations > 0 = throughput mode (Counter only), 0 = the handle's
 * checkers.  T_out: 16 floats per reading; stats / status: one entry per reading (status may be NULL: the first error is
 * then the return value).  1 <= batch <= 16.  Chains the batched kernels do not serve (knn > 1, several quantile filters,
 * SurfaceNormalOutlierFilter, unbounded maxDist) are registered one reading after the other -- same results. */
icpmi_status icpmi_register_batch_dev(icpmi_handle h, int32_t batch, const float* const* d_scans4, const int64_t* n,
                                      int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status);

/* ---- stage-level entry points (the per-stage virtuals of SURVEY.md 8b B2; used by parity tests) ---- */

/* `Transformation::compute(cloud, T)` (Mapper.cpp:197,221; Map.cpp:523,525): out4 = T * in4;
 * normals (3 x n, may be NULL) are rotated by the top-left 3x3. Rejects |1 - det R| > 1e-3
 * (TransformationError) with ICPMI_ERR_INVALID_ARG. */
icpmi_status icpmi_transform(icpmi_handle h, const float T[16], const float* in4, int64_t n, float* out4,
                             const float* in_normals3, float* out_normals3);

/* `Matcher::findClosests` == `Nabo::NNS::knn` against the CENTRED map of the handle
 * (queries are given in the centred frame). ids: k x n int32 (-1 unfilled, ORIGINAL map indices),
 * d2: k x n float (+inf unfilled), ascending by (d2, id). allow_self = 0 reproduces optionFlags = 0
 * of PointDistanceMapperModule.cpp:36. max_dist may be +inf. */
icpmi_status icpmi_knn(icpmi_handle h, const float* q4, int64_t n, int32_t k, float max_dist, int32_t allow_self,
                       int32_t* ids, float* d2);
/* `KDTreeVarDistMatcher::findClosests`: the same search and the same outputs with one radius per query (radii: n floats, host pointer,
 * each >= 0 or +inf; see icpmi_set_reading_max_dist).  radii == NULL: ICPMI_ERR_INVALID_ARG.  Works on any handle; a row armed by
 * icpmi_set_reading_max_dist is left alone. */
icpmi_status icpmi_knn_var(icpmi_handle h, const float* q4, int64_t n, int32_t k, const float* radii, int32_t allow_self,
                           int32_t* ids, float* d2);

/* `OutlierFilters::compute` for the handle's chain on given matches (host arrays, k x n; ids = ORIGINAL map indices, needed by
 * SurfaceNormal / GenericDescriptor / Robust; read_normals3 = the reading's `normals`, 3 x n, needed by SurfaceNormalOutlierFilter,
 * whose map side comes from the normals handed to icpmi_set_map). */
icpmi_status icpmi_outlier_weights(icpmi_handle h, const float* d2, const int32_t* ids, int32_t k, int64_t n,
                                   const float* read_normals3, float* weights, float* limit_out);

/* `ErrorMinimizer::compute`: one minimisation step for a reading given in the centred map frame,
 * with T_iter applied on the device first (T_iter may be NULL = identity). Runs NN + outlier
 * filters + minimiser of the handle's chain once. Outputs: T_step (4x4), and for inspection
 * sums[32] (double): point-to-plane -> A (upper 21, row-major packed) then b (6); point-to-point ->
 * sum w, sum w p (3), sum w q (3), sum w q p^T (9). Any output pointer may be NULL.
 * icpmi_config::degeneracy_threshold is honoured: T_step is the constrained step when it is > 0, and icpmi_get_localizability
 * afterwards reports this step's system (c0 and L are those of reading4 as given). */
icpmi_status icpmi_minimize_step(icpmi_handle h, const float* reading4, int64_t n, const float* T_iter,
                                 float T_step[16], double sums[32], icpmi_stats* stats);
/* ... with the reading's `normals` (read_normals3: 3 per point, the frame of reading4; rotated by T_iter on the device).  Serves every
 * minimiser: ICPMI_MIN_PLANE_TO_PLANE needs them (NULL: ICPMI_ERR_MISSING_NORMALS), for the others they feed
 * SurfaceNormalOutlierFilter only (which icpmi_minimize_step refuses) and NULL makes the call icpmi_minimize_step. */
icpmi_status icpmi_minimize_step_normals(icpmi_handle h, const float* reading4, int64_t n, const float* read_normals3, const float* T_iter,
                                         float T_step[16], double sums[32], icpmi_stats* stats);

/* epsilon of ICPMI_MIN_PLANE_TO_PLANE's covariances C(n) = I - (1 - eps) n n^T: finite, 0 < eps <= 1 (else ICPMI_ERR_INVALID_ARG and the
 * value stays); default 1e-3.  State of the handle: icpmi_set_config leaves it.  It is part of what a cached loop graph is valid for, so the
 * next registration runs with the new value.  eps = 1 makes every covariance I: A = 0.5 sum w J^T J. */
icpmi_status icpmi_set_plane_epsilon(icpmi_handle h, float eps);
icpmi_status icpmi_get_plane_epsilon(icpmi_handle h, float* eps);

/* The pair model that minimizer == ICPMI_MIN_PLANE_TO_PLANE runs.  State of the handle next to epsilon: icpmi_set_config leaves it, a cached
 * loop graph is valid for one model only, anything but the two values is ICPMI_ERR_INVALID_ARG and the state stays.
 *
 * ICPMI_PLANE_MODEL_SYMMETRIC -- SymmetricPointToPlaneErrorMinimizer{force4DOF}: the symmetric point-to-plane objective of S. Rusinkiewicz,
 * "A Symmetric Objective Function for ICP", ACM Trans. Graph. 38(4) (SIGGRAPH 2019), in its rotated-normals form: the normals are frozen per
 * iteration and the step is the ordinary linear one (no split rotation).  Not libpointmatcher's.  Per pair with weight w != 0: p = T_iter x,
 * q its match, u_q = n_q / |n_q|, u_p = R n_x / |R n_x| (R of T_iter; a zero or non-finite normal: u = 0), c = u_q . u_p, and the pair normal
 *     n_s = ( |c| u_q + c u_p ) / 2            (u_p = 0: n_s = u_q, which is point-to-plane; u_q = 0: n_s = u_p; both 0: the pair only counts)
 * then the point-to-plane sums with n_s for the normal: F = [p x n_s; n_s], A += w F F^T, b -= w F ((p - q) . n_s); per-pair terms in float,
 * the weight's product and the sums in double.  n_s is continuous in both normals (perpendicular ones weigh the pair down to a quarter),
 * the sign of either normal cancels bit for bit (unoriented normals are fine), u_q = u_p gives point-to-plane with the unit map normal, and
 * with c ~ 1 the residual is (p - q) . (n_q + n_p) / 2, which vanishes for two points of a surface of constant curvature.
 * Everything else is ICPMI_MIN_PLANE_TO_PLANE's: the slots of the sums, the solve with force4DOF, the entry points that serve it and those that
 * refuse it (their message names this minimiser), the rejected options (planar mode, covariance, degeneracy_threshold), the point-to-plane
 * residual of icpmi_residual_error*.  plane epsilon is ignored by this model, and kept. */
typedef enum {
    ICPMI_PLANE_MODEL_GICP = 0,     /* PlaneToPlaneErrorMinimizer: generalized ICP (the default) */
    ICPMI_PLANE_MODEL_SYMMETRIC = 1 /* SymmetricPointToPlaneErrorMinimizer                        */
} icpmi_plane_pair_model;
icpmi_status icpmi_set_plane_pair_model(icpmi_handle h, int32_t model);
icpmi_status icpmi_get_plane_pair_model(icpmi_handle h, int32_t* model);

/* VoxelMatcher: voxelised plane-to-plane ICP with no neighbour search (Koide et al., ICRA 2021; one voxel per reading point, the
 * "DIRECT1" neighbourhood).  Not a libpointmatcher module.  The resident map keeps one record per occupied voxel of its
 * CENTRED frame (points minus icpmi_get_map_mean): count, mean mu and N = (1/count) sum u u^T over the unit normals u of its points (a zero
 * or non-finite normal adds nothing).  A reading point p = T_iter x is paired with the voxel it falls into -- one table lookup, no voxel:
 * no pair -- with q = mu and M = (C_v + C(R n_x))^-1, C_v = I - (1 - eps) N, C(n) and eps as for ICPMI_MIN_PLANE_TO_PLANE; weight 1 per
 * pair.  The sums, the solve, the checkers and force_4dof are that minimiser's.  One iteration is two launches: no matcher, no selection.
 *   Keys: per axis i = (int)floorf(x / size) in float32 (correctly rounded division); a point takes part iff its coordinates are finite
 *   and every |i| < 2^20.  A MAP point that fails makes the build fail with ICPMI_ERR_INVALID_ARG; a reading point that fails has no pair.
 *   key = (i_x + 2^20) << 42 | (i_y + 2^20) << 21 | (i_z + 2^20).  The lookup is an open-addressing table with linear probing, capacity the
 *   smallest power of two >= max(2, 2 * voxels), a key's first slot = ((key * 0x9E3779B97F4A7C15 mod 2^64) >> 32) & (capacity - 1).
 *   Sums are in double in a fixed order and rounded once; no float atomics: two builds of one map give the same bits.
 * icpmi_set_voxel_matcher: size finite and >= 0 (else ICPMI_ERR_INVALID_ARG and the value stays).  0, the default, is off: no result changes
 * by a bit and no new kernel runs.  Handle state like the plane epsilon: icpmi_set_config leaves it.  The table is built lazily, by the
 * first call that needs it after the map or the size changed; a map without normals: ICPMI_ERR_MISSING_NORMALS.
 * With size > 0 on an ICPMI_MIN_PLANE_TO_PLANE handle with ICPMI_PLANE_MODEL_GICP, icpmi_register, _dev, _fixed_dev and
 * icpmi_minimize_step_normals run the voxel path (the reading must carry normals: ICPMI_ERR_MISSING_NORMALS); icpmi_config's knn, max_dist
 * and epsilon are not read by the loop; no pair at all is ICPMI_ERR_NO_POINT_TO_MINIMIZE; the sensor-noise overlap is not computed (-1).
 * Refused with a message that names the voxel matcher, never served by another path in silence:
 *   ICPMI_ERR_INVALID_ARG ("InvalidParameter: ..."): every other minimiser, the symmetric pair model, any outlier filter, var_dist, a
 *     non-zero intensity weight, covariance, degeneracy_threshold, force_2d / is_2d;
 *   ICPMI_ERR_UNSUPPORTED: icpmi_register_batch_dev, icpmi_register_multistart*, icpmi_register_sweep*, icpmi_sweep_sums, icpmi_minimize_step.
 * icpmi_residual_error* are unchanged: they score the pose through the nearest-neighbour matcher, as on any plane-to-plane handle.
 * icpmi_get_voxel_map: the table in ascending key order (builds it if need be).  ijk3 (3 per voxel), mean3 (3, centred frame), moments6
 *   (xx xy xz yy yz zz) and count have capacity cap voxels and may each be NULL; *n_voxels = the count; cap below it:
 *   ICPMI_ERR_INVALID_ARG with *n_voxels set.
 * icpmi_voxel_lookup (test seam and inspection): for n centred-frame queries (x, y, z, w) the index into that order, -1 for no voxel. */
icpmi_status icpmi_set_voxel_matcher(icpmi_handle h, float size);
icpmi_status icpmi_get_voxel_matcher(icpmi_handle h, float* size);
icpmi_status icpmi_get_voxel_map(icpmi_handle h, int64_t cap, int32_t* ijk3, float* mean3, float* moments6, int32_t* count, int64_t* n_voxels);
icpmi_status icpmi_voxel_lookup(icpmi_handle h, const float* q4_centred, int64_t n, int32_t* voxel);
/* diagnostics (scripts/voxel_bench.py): rebuilds the table and reports the milliseconds of its sort, reduce and fill stages */
icpmi_status icpmi_debug_voxel_build_times(icpmi_handle h, float times_ms3[3]);
/* ... and looks n centred-frame queries up `reps` times through the table (ms2[0]: mean milliseconds of one launch) and by a binary search over
 * the sorted keys (ms2[1]); *mismatch (may be NULL) = queries the two answer differently (0) */
icpmi_status icpmi_debug_voxel_lookup_times(icpmi_handle h, const float* q4_centred, int64_t n, int32_t reps, float ms2[2], int64_t* mismatch);

/* A schedule of voxel sizes: coarse-to-fine registration on the voxel path.  sizes[0..n) with n in 0..4, every size finite
 * and > 0, strictly descending (coarsest first); anything else: ICPMI_ERR_INVALID_ARG ("InvalidParameter: ...") and the schedule stays.
 * n = 0 switches the matcher off; n = 1 is icpmi_set_voxel_matcher(sizes[0]), bit for bit; icpmi_set_voxel_matcher(size) is a schedule of
 * one (or none at 0), and icpmi_get_voxel_matcher answers the finest size.
 * Level l uses the table of sizes[l], built by the one build path (its sorted records are bit for bit those of a one-size handle with that
 * size), lazily, and rebuilt when the map, its normals or the schedule change.  A level costs 64 B x its table's capacity.
 * A registration starts at level 0 and runs each level as an ICP run of its own on the chain's checkers: the Differential checker's history
 * and the Counter start afresh at each level (max_iterations bounds a LEVEL, the registration is bounded by levels x that count; the
 * history of a level after the first begins empty -- the pose carried over is not an entry, so such a level runs at least
 * smooth_length + 1 iterations); a stop by
 * either at a level before the last moves on to the next level with the pose unchanged; at the last level it ends the registration as on
 * a one-size handle.  The Bound checker (measured from the registration's start) and a level with no pair
 * (ICPMI_ERR_NO_POINT_TO_MINIMIZE) end the registration at once.  icpmi_register_fixed_dev runs its count at EVERY level.  The level
 * switch happens on the device, inside the one enqueued loop: no host wait between levels.  icpmi_stats::iterations is the total.
 * A schedule widens the basin of the finest size; it does not guarantee it: a level whose size divides the scene's own dimensions can have
 * a false minimum, and a schedule that starts there stays there (DESIGN.md 4.21 has the measured case).
 * Everything refused on a one-size handle is refused on a scheduled one, with the same messages.
 * icpmi_get_voxel_map and icpmi_voxel_lookup answer for the finest level, the _level variants for level `level` (0 = the coarsest; no such
 *   level: ICPMI_ERR_INVALID_ARG).
 * icpmi_get_voxel_schedule_report (two or more levels, else ICPMI_ERR_INVALID_ARG): of the handle's last registration, *levels = the levels
 *   entered, and per level the iterations run and the pair counts of its first and of its last iteration (0 for a level not entered; a
 *   level that found no pair reports 0 iterations and 0 pairs).
 * icpmi_minimize_step_normals on a scheduled handle evaluates at the finest level; icpmi_debug_voxel_step_level (test seam) selects
 *   another, -1 the finest again; a new schedule resets it. */
icpmi_status icpmi_set_voxel_schedule(icpmi_handle h, const float* sizes, int32_t n);
icpmi_status icpmi_get_voxel_schedule(icpmi_handle h, float sizes[4], int32_t* n);
icpmi_status icpmi_get_voxel_map_level(icpmi_handle h, int32_t level, int64_t cap, int32_t* ijk3, float* mean3, float* moments6, int32_t* count,
                                       int64_t* n_voxels);
icpmi_status icpmi_voxel_lookup_level(icpmi_handle h, int32_t level, const float* q4_centred, int64_t n, int32_t* voxel);
icpmi_status icpmi_get_voxel_schedule_report(icpmi_handle h, int32_t* levels, int32_t iterations[4], int32_t pairs_first[4], int32_t pairs_last[4]);
icpmi_status icpmi_debug_voxel_step_level(icpmi_handle h, int32_t level);

/* Many poses scored by table lookup, for relocalisation on the voxel path.  No matcher launch, no selection, no tile sort.
 * Reading, T and the frame mean what they mean for icpmi_residual_error: the reading as given, T[p] (16 floats, column-major) a correction
 * in the map frame; the centred pose Tc = [R | t + R mu - mu] is formed in double on the host.  Per reading point x (x, y, z, w), its
 * normal n_x and pose, in float32 with no contraction, exactly voxel_pairs_kernel's arithmetic up to S:
 *   p   = Tc x                 per row r: fmaf(Tc[12+r], w, fmaf(Tc[8+r], z, fmaf(Tc[4+r], y, Tc[r] * x)))
 *   key = the float32 floor of p / size (above); no voxel: no pair, the point adds nothing
 *   d   = p - mu;  u = unit_or_zero(R n_x), row r of R n_x = fmaf(Tc[8+r], n.z, fmaf(Tc[4+r], n.y, Tc[r] * n.x)); g = 1 - eps
 *   S   = 2 I - g (N + u u^T):  sxx = 2 - g * (Nxx + u.x * u.x) (likewise syy, szz), sxy = -g * (Nxy + u.x * u.y) (likewise sxz, syz)
 *   M   = adj(S) / det(S):  c00 = syy * szz - syz * syz, c01 = sxz * syz - sxy * szz, c02 = sxy * syz - sxz * syy, c11 = sxx * szz - sxz * sxz,
 *         c12 = sxy * sxz - sxx * syz, c22 = sxx * syy - sxy * sxy, idet = 1 / ((sxx * c00 + sxy * c01) + sxz * c02), m_ij = c_ij * idet
 *   Md  = ((m00 * d.x + m01 * d.y) + m02 * d.z,  (m01 * d.x + m11 * d.y) + m12 * d.z,  (m02 * d.x + m12 * d.y) + m22 * d.z)
 *   r   = (d.x * Md.x + d.y * Md.y) + d.z * Md.z
 *   l   = expf(-(hb * r)),  hb = 0.5f * beta rounded once on the host
 * Per pose, in double, in a fixed order that depends on n alone (no float atomics): pairs, likelihood = sum l, sum_maha = sum r; max_maha =
 * the largest r (float, exact; 0 without a pair); pairs_ratio = (float)(pairs / n); level = the level scored.  The reading is cut into
 * slices of *slice points (icpmi_voxel_score_shape), a thread adds its points in ascending order, a wave folds by the xor butterfly
 * (partners 1, 2, .. 32), the waves and then the slices add in ascending order.  A bounded likelihood ranks poses where the mean of r does
 * not: it joins "how many points fall on the map" and "how well they fit".
 * out[p] and status[p] are bit for bit what a call with pose p alone returns, whichever poses share the call and in whatever order.
 * Errors of the whole call, found before anything is enqueued, with out and status zeroed (min(n_poses, 4096) entries): a handle that is not on the voxel path
 * (ICPMI_ERR_UNSUPPORTED); no map, null arguments, n < 0, n_poses outside 1 .. 4096, a level the schedule does not have, beta not finite or
 * <= 0 (ICPMI_ERR_INVALID_ARG); a map without normals or no reading normals (ICPMI_ERR_MISSING_NORMALS); n == 0
 * (ICPMI_ERR_NO_POINT_TO_MINIMIZE).  Errors of one pose go to status[p] (status == NULL: the first of them is the return value): a T[p] that
 * is not rigid (ICPMI_ERR_INVALID_ARG; not launched, out[p] zero), pairs == 0 (ICPMI_ERR_NO_POINT_TO_MINIMIZE).
 * The one-shot reading rows are consumed.  Afterwards the handle is as after icpmi_voxel_lookup: no registration result, covariance,
 * schedule report, staged scan or captured loop has changed.  icpmi_voxel_score_poses uploads the reading once. */
typedef struct { int32_t level; float beta; int32_t reserved[6]; } icpmi_voxel_score_options;
/* level -1: the last (finest) level, and the only one of a one-size handle; beta 1 */
typedef struct { double likelihood; double sum_maha; int64_t pairs; float max_maha; float pairs_ratio; int32_t level; int32_t reserved[3]; } icpmi_voxel_score;
void icpmi_voxel_score_options_default(icpmi_voxel_score_options* opts);
void icpmi_voxel_score_shape(int32_t* slice, int32_t* tile); /* points per slice, poses a workgroup walks */
icpmi_status icpmi_voxel_score_poses_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, const float* T,
                                         int32_t n_poses, const icpmi_voxel_score_options* opts, icpmi_voxel_score* out, icpmi_status* status);
icpmi_status icpmi_voxel_score_poses(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float* T, int32_t n_poses,
                                     const icpmi_voxel_score_options* opts, icpmi_voxel_score* out, icpmi_status* status);

/* Many readings, or many starts of one reading, registered in one loop on the voxel path.  The handle is a VoxelMatcher
 * handle, one-size or scheduled.  icpmi_register_batch_dev and icpmi_register_multistart* keep refusing such a handle: they cannot carry
 * the readings' normals.
 * icpmi_voxel_register_batch_dev: batch in 1 .. 16 readings d_scans4[b] (device, n[b] points of 4 floats) with their normals
 *   d_scan_normals3[b] (device, 3 floats per point).  T_out + 16 b, status[b] and stats[b] are bit for bit what
 *   icpmi_register_dev(h, d_scans4[b], n[b], d_scan_normals3[b], ...) -- fixed_iterations > 0: icpmi_register_fixed_dev -- returns for that
 *   reading alone, whichever readings share the launch and in whatever order.  Outside that claim are the timing fields of icpmi_stats:
 *   loop_ms (the whole batch's loop here), nn_ms_avg and nn_launches.  status == NULL: the first error of a member is the return value.
 * icpmi_voxel_register_multistart_dev: one reading and n_starts in 1 .. 16 priors (16 floats each, column-major).  Reading and normals are
 *   moved by every prior on the device into slices of their own, with icpmi_transform's arithmetic element for element, and the slices
 *   go through the batch: start s is bit for bit icpmi_transform(priors + 16 s) followed by icpmi_register on the result.  T_out + 16 s is
 *   the correction that registration returns (composing it with the prior stays the caller's).  A prior that is not rigid:
 *   ICPMI_ERR_INVALID_ARG in status[s], an identity, the other starts untouched.  icpmi_voxel_register_multistart takes host pointers and
 *   uploads the reading and its normals once.
 * icpmi_get_voxel_batch_report: member b's (start s's) icpmi_get_voxel_schedule_report for the last of these calls;
 *   ICPMI_ERR_INVALID_ARG on a handle with fewer than two levels or for a member that call did not have.
 * Errors of the whole call, found before anything is enqueued, with T_out set to identities: batch / n_starts outside 1 .. 16, null
 *   arguments, n < 0 (ICPMI_ERR_INVALID_ARG); a handle that is not on the voxel path (ICPMI_ERR_INVALID_ARG, the message names
 *   icpmi_set_voxel_matcher); everything a single registration on the voxel path refuses, in its words; a member with points and no
 *   normals pointer (ICPMI_ERR_MISSING_NORMALS).  An empty map: identities and ICPMI_OK.
 * A batch of one, or one with an empty member (n[b] == 0), registers its members one after the other: the same answers, no sharing.
 * Afterwards: no covariance, no staged scan, nothing for icpmi_debug_last_matches; the one-shot reading rows are consumed. */
icpmi_status icpmi_voxel_register_batch_dev(icpmi_handle h, int32_t batch, const float* const* d_scans4, const int64_t* n,
                                            const float* const* d_scan_normals3, int32_t fixed_iterations, float* T_out, icpmi_stats* stats,
                                            icpmi_status* status);
/* ... for readings and normals on the host (what the C++ host shell calls): one upload per reading, then the call above */
icpmi_status icpmi_voxel_register_batch(icpmi_handle h, int32_t batch, const float* const* scans4, const int64_t* n,
                                        const float* const* scan_normals3, int32_t fixed_iterations, float* T_out, icpmi_stats* stats,
                                        icpmi_status* status);
icpmi_status icpmi_voxel_register_multistart_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, const float* priors,
                                                 int32_t n_starts, int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status);
icpmi_status icpmi_voxel_register_multistart(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float* priors,
                                             int32_t n_starts, int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status);
icpmi_status icpmi_get_voxel_batch_report(icpmi_handle h, int32_t member, int32_t* levels, int32_t iterations[4], int32_t pairs_first[4],
                                          int32_t pairs_last[4]);
/* test seam: out[0] = loops the voxel batch has run on this handle, out[1] = the members they carried, out[2] = single registrations on the
 * voxel path (icpmi_register*, and the one-by-one route of the calls above) */
icpmi_status icpmi_debug_voxel_batch_calls(icpmi_handle h, int64_t out[3]);

/* ---- Global localisation: branch and bound over voxel occupancy levels (the 3D-BBS formulation of Aoki, Koide, Oishi,
 * Yokozuka, Banno, ICRA 2024).  A search without candidates: exhaustive over a lattice of translations and a caller-supplied list of
 * rotations, exact, all in integers.  It needs no normals on either cloud and no matcher, and works on any handle that holds a map.
 *
 * Frame and cells.  Points live in the handle's centred frame, mu = icpmi_get_map_mean.  s0 (finite, > 0, float32) is the finest cell size.
 *   Cells are those of the voxel table above: per axis (int)floorf(x / s0) in float32, taking part iff finite and |i| < 2^19 -- half of the
 *   table's range, so that cell plus offset always fits the 63-bit key.  A map point out of that range: ICPMI_ERR_INVALID_ARG.
 *   occ0 = the set of cells of the resident map's points.
 * Poses.  Rotation k of the list is R_k: R9 + 9 k, column-major 3 x 3 (R[r][c] = R9[9 k + 3 c + r]).  The translation is tau = mu + s0 * a
 *   with integer a in a window [a_min, a_max] per axis; the pose [R_k | tau] is a correction in the map frame, as T is elsewhere.
 *   For a reading point x (x, y, z, w; w not used) y = R_k x, per row r in float32 with no contraction:
 *     fmaf(R[r][2], z, fmaf(R[r][1], y, R[r][0] * x)),  c = floorf(y / s0) per axis.
 *   A point whose y is not finite, or with |c| >= 2^19 on an axis, adds nothing under that rotation.
 * Score.  score(k, a) = the number of reading points with c + a in occ0 (int64).
 * Levels l = 0 .. L-1, L in 1 .. 8.  A node (k, l, A) stands for the 2^l cube of translations a in [A * 2^l, A * 2^l + 2^l - 1] per axis.
 *   bound(k, l, A) = the number of points with (c >> l) + A in occB_l (>> = the arithmetic shift, floor division), where
 *   occC_l = { u >> l : u in occ0 }, occB_0 = occ0, and for l >= 1 occB_l = { w - e : w in occC_l, e in {0, 1}^3 }.
 *   For a in the node's cube (c + a) >> l is (c >> l) + A or that plus one per axis, so occ0[c + a] <= occB_l[(c >> l) + A]: the bound is
 *   at least the largest score in the cube, and bound(k, 0, a) = score(k, a).
 * Tables.  Per level the keys of occB_l ascending (icpmi_get_occupancy_level hands them out as cells, with icpmi_get_voxel_map's capacity
 *   rule; cap == 0 with ijk3 == NULL is a size query: *n_keys alone, ICPMI_OK) and an open-addressing table of key-only 8-byte slots: capacity the smallest power of two >= 2 x keys, first slot
 *   (key * 0x9E3779B97F4A7C15 >> 32) & (capacity - 1), linear probing.  Built lazily on the device and kept on the handle for (map, s0): a level
 *   depends on (map, s0, l) alone, so a pyramid of fewer levels is extended and one of more serves a call that asks for fewer.
 * Window.  options.box_lo / box_hi (has_box != 0): a box in the map frame in metres; a_min = floor((lo - mu) / s0), a_max =
 *   floor((hi - mu) / s0), formed in double.  lo <= hi, finite, |a| < 2^19, else ICPMI_ERR_INVALID_ARG.  Without a box the window is the
 *   map's bounding box in cells: the smallest and the largest cell of occ0 per axis.  Top-level nodes are the blocks A in
 *   [a_min >> (L-1), a_max >> (L-1)] of every rotation; a child whose cube does not meet the window is dropped unscored, a leaf outside
 *   the window is no candidate.
 * Search.  Best-first and batched.  A heap ordered by (bound descending, level ascending, k ascending, A lexicographic).  The top-level
 *   nodes are scored in launches of at most *launch_nodes nodes (icpmi_global_localize_shape).  Then rounds: pop up to `batch` nodes whose
 *   bound is > best; form their window-clipped children (at most 8 each); score all of them in one launch, read the counts back once; the
 *   first leaf in the heap's order becomes the best if its score is > best (strictly: the first in that order wins a tie); push every
 *   inner child with bound > best.  It stops when the heap's top is <= best.  The answer is the same for every batch; nodes_scored is
 *   not, and is a function of (map, reading, rotations, options) alone.
 *   levels 0 = automatic: the largest L <= 6 with 2^(L-1) at most the window's longest side in cells, at least 1.
 *   min_score_ratio (default 0): need = ceil((double)(float)ratio * n); the search starts with best = need - 1 and answers found = 0
 *   (ICPMI_OK) when nothing reaches need: what keeps a reading that is not in the map from costing more than the exhaustive search.
 *   max_nodes (default 0: no cap): checked behind every launch; once more nodes than that have been scored the search stops with the best
 *   so far and proven = 0.  batch: 1 .. 8192 (default 64): a round's children, at most 8 each, fit one launch.
 *   A larger batch means fewer, fuller launches and more nodes scored (DESIGN.md 4.24 has both measured); the default is provisional.
 * Result.  found; proven (the search ran to its end); rotation k, cell a, score; points = the points that took part under R_k; T =
 *   [R_k | tau] column-major, tau = (double)mu + (double)s0 * a rounded once to float; levels = L; nodes_scored, leaves_scored, launches
 *   (scoring launches).  found = 0: rotation -1, T the identity.
 * icpmi_occupancy_score_nodes (test seam and inspection): bound(k, l, A) of n_nodes caller-given nodes, 5 ints each (k, l, A.x, A.y, A.z)
 *   with k in [0, n_rot), l in [0, levels), |A| < 2^19, through the kernel the search uses; `levels` in 1 .. 8.
 * Errors of the whole call, found before anything is enqueued, with the result zeroed: no map, null arguments, n < 0, n_rot outside
 *   1 .. 4096, a rotation that is not orthonormal (the test of icpmi_transform), s0 not finite or <= 0, levels outside 0 .. 8, batch outside
 *   1 .. 8192, a negative max_nodes, a min_score_ratio that is not finite or outside 0 .. 1, a bad box (ICPMI_ERR_INVALID_ARG); n == 0
 *   (ICPMI_ERR_NO_POINT_TO_MINIMIZE); planar mode, force_2d or is_2d (ICPMI_ERR_UNSUPPORTED, the message names the call).
 * Afterwards the handle is as after icpmi_voxel_lookup: no registration result, covariance, staged scan or captured loop has changed, and
 *   the VoxelMatcher tables are neither read nor touched.  icpmi_global_localize uploads the reading once. */
typedef struct {
    float cell_size; int32_t levels; float min_score_ratio; int32_t batch; int64_t max_nodes; int32_t has_box; int32_t reserved0;
    double box_lo[3]; double box_hi[3]; int32_t reserved[8];
} icpmi_global_localize_options;
typedef struct {
    int32_t found; int32_t proven; int32_t rotation; int32_t cell[3]; int64_t score; int64_t points; float T[16]; int32_t levels;
    int32_t launches; int64_t nodes_scored; int64_t leaves_scored; int32_t reserved[8];
} icpmi_global_localize_result;
void icpmi_global_localize_options_default(icpmi_global_localize_options* opts); /* cell_size 0.5, levels 0, ratio 0, batch 64, no cap, no box */
void icpmi_global_localize_shape(int32_t* slice, int32_t* tile, int32_t* launch_nodes); /* points per slice, nodes a workgroup walks, nodes per launch */
icpmi_status icpmi_global_localize(icpmi_handle h, const float* scan4, int64_t n, const float* R9, int32_t n_rot,
                                   const icpmi_global_localize_options* opts, icpmi_global_localize_result* result);
icpmi_status icpmi_global_localize_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* R9, int32_t n_rot,
                                       const icpmi_global_localize_options* opts, icpmi_global_localize_result* result);
icpmi_status icpmi_occupancy_score_nodes(icpmi_handle h, const float* scan4, int64_t n, const float* R9, int32_t n_rot, float s0, int32_t levels,
                                         const int32_t* nodes5, int64_t n_nodes, int64_t* counts);
icpmi_status icpmi_get_occupancy_level(icpmi_handle h, float s0, int32_t levels, int32_t level, int64_t cap, int32_t* ijk3, int64_t* n_keys);
/* inspection (scripts/global_localize_bench.py): of the pyramid the handle holds, *levels, and per level the keys, the bytes of keys and
 * table, and the host milliseconds its build took; *builds = pyramids built on this handle so far.  Every pointer may be NULL. */
icpmi_status icpmi_get_occupancy_info(icpmi_handle h, int32_t* levels, int64_t keys[8], int64_t bytes[8], float build_ms[8], int64_t* builds);

/* ---- IntensityPointToPlaneErrorMinimizer: a photometric term on ICPMI_MIN_POINT_TO_PLANE.  Not libpointmatcher's: the joint
 * geometric + photometric objective of Park, Zhou, Koltun, "Colored Point Cloud Registration Revisited" (ICCV 2017), one scalar channel.
 *
 * Map side, once per map: for every map point i with unit normal u = n_i / |n_i| an intensity gradient g_i in its tangent plane, from its K
 * nearest OTHER map points j (the self search of icpmi_surface_normals with k = K + 1, the point itself first; 1 <= K <= 31; unfilled slots and
 * neighbours with a non-finite intensity are skipped):  e1 = normalise(u x axis), axis = the coordinate axis of the smallest |u| component,
 * e2 = u x e1;  d = (x_j - x_i) - u (u . (x_j - x_i)), a = d . e1, b = d . e2, dI = I_j - I_i;  S = sum [a b]^T [a b], r = sum [a b]^T dI in float,
 * neighbour order;  g2 = S^-1 r in closed form, g_i = g2.x e1 + g2.y e2.  g_i = 0 when the normal is zero or non-finite, I_i is non-finite, fewer
 * than 2 neighbours are usable, or det S <= 1e-4 (tr S / 2)^2 (the neighbours lie on a line, or on the point).
 *
 * Per pair with weight w != 0 (p = T_iter x, q its match with normal n as the point-to-plane sums read it, (g, I_q) of the match, I_p of the
 * reading point), lambda = 1 - weight:
 *     r_G = (p - q) . n,  F_G = [p x n; n]                                   (the point-to-plane terms, bit for bit)
 *     m = g - n (g . n),  p' = p - n r_G,  r_I = I_q + g . (p' - q) - I_p,  F_I = [p x m; m]
 *     A += w (lambda F_G F_G^T + (1 - lambda) F_I F_I^T),   b -= w (lambda F_G r_G + (1 - lambda) F_I r_I)
 * per-pair terms in float, the weight's products and the sums in double, in the point-to-plane slots of sums[32]; a pair whose I_p or I_q is
 * non-finite adds the geometric part only; sums[27] and sums[28] are point-to-plane's.  Intensities are taken as given: scaling them by s acts
 * like a photometric weight s^2.
 *
 * icpmi_set_intensity_weight: w = 1 - lambda, finite, 0 <= w < 1 (else ICPMI_ERR_INVALID_ARG and the value stays).  0, the default, is off: no
 * result changes by a bit and no other kernel runs.  State of the handle next to the plane epsilon: icpmi_set_config leaves it, and it is
 * part of what a cached loop graph is valid for.  With w > 0:
 *   - icpmi_register, _dev, _fixed_dev, icpmi_register_prior*, icpmi_minimize_step and icpmi_minimize_step_normals serve the term.  They need
 *     the map's channel and the reading's row: without either, ICPMI_ERR_INVALID_ARG with "InvalidField: ..." naming the missing setter;
 *   - every minimizer but ICPMI_MIN_POINT_TO_PLANE, force_2d / is_2d, covariance = 1 and degeneracy_threshold != 0 are refused by those entry
 *     points, and icpmi_register_batch_dev, icpmi_register_multistart*, icpmi_register_sweep* / icpmi_sweep_sums refuse the handle
 *     (ICPMI_ERR_UNSUPPORTED, the message names the term);
 *   - icpmi_residual_error* report the point-to-plane residual, unchanged. */
icpmi_status icpmi_set_intensity_weight(icpmi_handle h, float w);
icpmi_status icpmi_get_intensity_weight(icpmi_handle h, float* w);
/* The resident map's intensity, one value per point in the caller's order (host pointer; m must equal the map's size: else
 * ICPMI_ERR_INVALID_ARG; a map without normals: ICPMI_ERR_MISSING_NORMALS; knn = K above).  Computes the gradients on the device and keeps
 * (g.x, g.y, g.z, I) per map point in the index's order.  Every call that changes the resident map (icpmi_set_map*, the map updates and chains,
 * inserts, epochs) drops the channel. */
icpmi_status icpmi_set_map_intensity(icpmi_handle h, const float* intensity, int64_t m, int32_t knn);
/* The intensity of the NEXT reading, one value per point in the caller's order: a one-shot row with the contract of icpmi_set_reading_scalar
 * (consumed by the next call that takes a reading, whatever becomes of it; n must match that reading). */
icpmi_status icpmi_set_reading_intensity(icpmi_handle h, const float* row, int64_t n);
/* The gradient operator by itself, on host pointers (pts4: 4 x m, normals3: 3 x m, intensity: m, grad3_out: 3 x m, knn = K): the kernel of
 * icpmi_set_map_intensity; touches no state of the handle but its private search handle, like icpmi_surface_normals. */
icpmi_status icpmi_intensity_gradient(icpmi_handle h, const float* pts4, int64_t m, const float* normals3, const float* intensity, int32_t knn,
                                      float* grad3_out);

/* ---- map-side operators on the path ---- */

/* `SurfaceNormalDataPointsFilter{knn}` (Map.cpp:524 via examples/config.yaml:26-27). */
icpmi_status icpmi_surface_normals(icpmi_handle h, const float* pts4, int64_t m, int32_t knn, float* normals3);
/* ... with `keepDensities: 1`: densities (m floats, may be NULL) = knn / (4/3 pi r^3), r = the largest distance of a neighbour
 * from the centroid of the neighbourhood (the descriptor MaxDensityDataPointsFilter reads). */
icpmi_status icpmi_surface_normals_ex(icpmi_handle h, const float* pts4, int64_t m, int32_t knn, float* normals3, float* densities);
/* (v4) ... with `keepMatchedIds: 1` / `keepMeanDist: 1`: matched_ids (knn x m int32, column i = the neighbours of point i by ascending
 * (d2, index), the point itself first; may be NULL) and mean_dist (m floats: distance from the point to the mean of its neighbours; may be NULL). */
icpmi_status icpmi_surface_normals_ex2(icpmi_handle h, const float* pts4, int64_t m, int32_t knn, float* normals3, float* densities,
                                       int32_t* matched_ids, float* mean_dist);
/* (r5) ... with `keepEigenValues: 1` / `keepEigenVectors: 1` and `sortEigen: 1`: eig_values3 (3 x m, may be NULL) = the eigenvalues of the
 * neighbourhood's scatter matrix NN NN^T in ascending order; eig_vectors9 (9 x m, may be NULL) = upstream's serializeEigVec of the
 * eigenvector matrix in that column order (entry 3 k + j of a point = component k of eigenvector j).  Rank < 2: zeros / identity, as upstream.
 * The sign of an eigenvector is the solver's.  Upstream's UNSORTED order (sortEigen: 0) is whatever Eigen::EigenSolver returns and is not
 * reproduced: the host filter serves the two descriptors only together with sortEigen: 1. */
icpmi_status icpmi_surface_normals_ex3(icpmi_handle h, const float* pts4, int64_t m, int32_t knn, float* normals3, float* densities,
                                       int32_t* matched_ids, float* mean_dist, float* eig_values3, float* eig_vectors9);

/* `PointDistanceMapperModule::inPlaceUpdateMap` keep mask (PointDistanceMapperModule.cpp:28-50):
 * keep[i] = 1 iff the exact NN of input i in map (self match excluded) has d2 >= min_dist^2. */
icpmi_status icpmi_point_distance_keep(icpmi_handle h, const float* map4, int64_t m, const float* in4, int64_t n,
                                       float min_dist, uint8_t* keep);

/* `Map::updateLocalPointCloud` for the PointDistance chain, on the resident map (Map.cpp:502-534 with
 * PointDistanceMapperModule.cpp:28-50 as the only module and, when normals_knn > 0, SurfaceNormalDataPointsFilter{knn}
 * as the post filter, examples/config.yaml:26-27): scan4 (n x 4, MAP frame) -> keep mask against the handle's current
 * map (self match excluded, keep iff d2 >= min_dist^2) -> kept points appended in input order -> normals of the whole
 * grown map recomputed (normals_knn > 0; else the appended points take scan_normals3 or zeros) -> index rebuilt
 * (`icp.setMap`, Map.cpp:528).  Only the scan crosses PCIe; keep_out (n bytes, may be NULL) receives the keep mask so
 * that a host that owns further descriptors of the map can append the kept rows itself.  On a handle without a map the scan becomes the map
 * (`PointDistanceMapperModule::createMap`).  The post filter runs in the map frame (the reference rotates the cloud
 * into the sensor frame and back, Map.cpp:523-525; PCA normals are rotation-equivariant up to rounding). */
icpmi_status icpmi_map_update_point_distance(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3,
                                             float min_dist, int32_t normals_knn, uint8_t* keep_out, int64_t* appended, int64_t* new_m);

/* `Mapper::processInput` with the scan staged once (Mapper.cpp:194-238): scan4 arrives in the SENSOR frame;
 * icpmi_register_prior moves it into the map frame by the prior on the device (`transformation->compute(input,
 * estimatedPose)`, :197), registers it (`icp(input)`, :213) and keeps that cloud in HBM; T_out is the correction.
 * If the update policy then asks for a map update, icpmi_map_update_staged applies the correction to the kept
 * cloud (`transformation->compute(input, correction)`, :221) and runs icpmi_map_update_point_distance on it --
 * the scan crosses PCIe once per processInput instead of five times. */
icpmi_status icpmi_register_prior(icpmi_handle h, const float* scan4, int64_t n, const float prior[16], float T_out[16],
                                  icpmi_stats* stats);
/* (v4) the same with the sensor-frame scan already in HBM on the handle's GPU: no PCIe crossing at all */
icpmi_status icpmi_register_prior_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float prior[16], float T_out[16],
                                      icpmi_stats* stats);
icpmi_status icpmi_map_update_staged(icpmi_handle h, const float correction[16], float min_dist, int32_t normals_knn,
                                     uint8_t* keep_out, int64_t* appended, int64_t* new_m);

/* `PointDistanceMapperModule` keep mask of the scan staged by icpmi_register_prior against the RESIDENT map, without
 * touching the map (scan-sharded mapping, SURVEY.md 8e: every rank decides which of its points are new, the accepted
 * points of all ranks are exchanged, and only then does every replica append the same set): the staged cloud is moved by
 * `correction` (Mapper.cpp:221); keep_out[i] = 1 iff its exact nearest map neighbour is at least min_dist away
 * (PointDistanceMapperModule.cpp:33-42); placed_out4 (n x 4, may be NULL) receives the moved cloud. */
icpmi_status icpmi_staged_point_distance_keep(icpmi_handle h, const float correction[16], float min_dist, uint8_t* keep_out,
                                              float* placed_out4);

/* Download of the resident map in the caller's order (what `Map::getLocalPointCloud` returns, Map.cpp:536-540);
 * out4 / normals3 may be NULL to query *m only. */
icpmi_status icpmi_get_map(icpmi_handle h, float* out4, float* normals3, int64_t capacity, int64_t* m);

/* `OctreeMapperModule::inPlaceUpdateMap` decimation (OctreeMapperModule.cpp:35-39 -> OctreeGridDataPointsFilter
 * {maxSizeByNode: edge, samplingMethod: 0}), as a lattice stand-in: voxel index floor((p - lo) / edge) per axis
 * with lo the bounding-box minimum; keep[i] = 1 iff i is the smallest index of its voxel. */
icpmi_status icpmi_voxel_keep_first(icpmi_handle h, const float* in4, int64_t n, float edge, uint8_t* keep);

/* `DynamicPointsMapperModule::inPlaceUpdateMap` (DynamicPointsMapperModule.cpp:34-172; parameters :6-13).
 * `to_sensor` = pose^-1 (col-major 4x4, :51,57); input4 / map4 in the map frame; map_normals3 = descriptor `normals`
 * of the map; prob_dynamic (m floats) = descriptor `probabilityDynamic` of the map, updated in place for every
 * map point within sensor_max_range that has an input beam within 2 * beam_half_angle in (elevation, azimuth).
 * beam_half_angle <= 0: ICPMI_ERR_INVALID_ARG; so small that the angular grid would need more than 2^28 buckets (below about 2.7e-4 rad):
 * ICPMI_ERR_UNSUPPORTED.  Either way nothing is touched -- in icpmi_map_update_chain too, where both are checked before the program starts. */
typedef struct icpmi_dynpts_params {
    float threshold_dynamic; /* 0.6  */
    float alpha;             /* 0.8  */
    float beta;              /* 0.99 */
    float beam_half_angle;   /* 0.01 rad */
    float epsilon_a;         /* 0.01 */
    float epsilon_d;         /* 0.01 m */
    float sensor_max_range;  /* 200 m */
} icpmi_dynpts_params;
icpmi_status icpmi_dynamic_points_update(icpmi_handle h, const icpmi_dynpts_params* prm, const float to_sensor[16],
                                         const float* input4, int64_t n, const float* map4, const float* map_normals3,
                                         int64_t m, float* prob_dynamic);

/* Same decimation with a choice of representative: method 0 = smallest index of the voxel (icpmi_voxel_keep_first),
 * method 1 = `samplingMethod: 1` (a random point of the voxel, examples/config.yaml:49) made reproducible: the point
 * whose index has the smallest 32-bit finaliser hash (fmix32 of MurmurHash3, a bijection) represents its voxel. */
icpmi_status icpmi_voxel_keep(icpmi_handle h, const float* in4, int64_t n, float edge, int32_t method, uint8_t* keep);

/* `SamplingSurfaceNormalDataPointsFilter{ratio, knn, samplingMethod: 0, maxBoxDim, seed}` -- the REFERENCE filter of
 * `PM::ICPSequence::setDefault()` (a configuration without an `icp:` key, Mapper.cpp:74-78), run at every `icp.setMap` (Map.cpp:111,178,528,581):
 * median splits of the widest box dimension (ties by index) until a box holds <= knn points, one PCA normal per box (boxes of rank < 2 or
 * wider than maxBoxDim are dropped), the points of a box -- in index order -- kept with probability ratio (std::minstd_rand seeded with
 * `seed`, one number per point of a surviving box, boxes in depth-first order).  order_out (capacity n) receives the kept indices in box
 * order, normals3_out (capacity 3 n) their normals; *n_out the number kept.  Entirely on the device (csrc/ssn.hip). */
icpmi_status icpmi_sampling_surface_normal(icpmi_handle h, const float* in4, int64_t n, float ratio, int32_t knn, float max_box_dim, int32_t seed,
                                           int32_t* order_out, float* normals3_out, int64_t* n_out);
/* ... with `samplingMethod` (upstream's fuseRange, as recalled): 0 = the call above (the extra outputs are not touched); 1 = every surviving box
 * is replaced by ONE point: order_out[j] = the smallest index of box j (the column the caller keeps), mean3_out[3 j ..] its new position -- the
 * mean of the box, accumulated in double in index order --, normals3_out[3 j ..] the box normal, and members_out[member_start_out[j] ..
 * + member_count_out[j]) the members of the box in index order: what `averageExistingDescriptors` averages over (descriptor rows live with
 * the caller).  No random number is drawn; boxes in depth-first order; *n_out = number of boxes.  Capacities n (3 n for mean3_out); any
 * of the four extra outputs may be NULL.  Entirely on the device. */
icpmi_status icpmi_sampling_surface_normal_ex(icpmi_handle h, const float* in4, int64_t n, float ratio, int32_t knn, float max_box_dim, int32_t seed,
                                              int32_t method, int32_t* order_out, float* normals3_out, int64_t* n_out, float* mean3_out,
                                              int32_t* member_start_out, int32_t* member_count_out, int32_t* members_out);

/* `OctreeGridDataPointsFilter{maxSizeByNode, maxPointByNode, samplingMethod}` (created at OctreeMapperModule.cpp:12, applied at :38):
 * octree over the bounding cube of the cloud, split until the node edge is <= max_size or the node holds <= max_points points
 * (depth capped at 21), one representative per leaf: method 0 = the first point of the leaf (smallest index), 1 = a random
 * point made reproducible (smallest fmix32(index)).  order_out (capacity n) = indices of the kept points in the order upstream
 * leaves the cloud in (depth-first leaf order); leaf_of_out (n entries, may be NULL) = leaf ordinal of every input point (for
 * callers that build centroids / medoids, samplingMethod 2 / 3, themselves). */
icpmi_status icpmi_octree_sample(icpmi_handle h, const float* in4, int64_t n, float max_size, int32_t max_points, int32_t method,
                                 int32_t* order_out, int32_t* leaf_of_out, int64_t* n_out);

/* `VoxelGridDataPointsFilter{vSizeX, vSizeY, vSizeZ, useCentroid: 1, averageExistingDescriptors}` (libpointmatcher
 * DataPointsFilters/VoxelGrid, AS RECALLED: upstream's source is not on hand; every quantity is float32, every division
 * correctly rounded, no contraction):
 *   minV / maxV = per-axis minimum / maximum of the coordinates; minB = minV / vsize, maxB = maxV / vsize;
 *   numDiv[a] = (unsigned)((1 + maxB[a]) - minB[a]) (left to right in float, then truncated);
 *   point p: i = (unsigned)floor(x_p / vsize[0] - minB[0]), j and k the same on y and z;
 *   idx = i + j numDiv[0] + k numDiv[0] numDiv[1] in unsigned 32-bit arithmetic.
 * The points of one idx form a voxel; its first point is the member with the smallest index.  Output: one point per voxel, in
 * ascending order of first-point index.  x, y, z = the centroid: the first point's value, plus every other member in ascending
 * index order (one float add at a time), divided by (float)count; the homogeneous row is the first point's.  Descriptors
 * (desc: point-major, n x desc_rows; NULL when desc_rows == 0): average_descriptors = 1 averages every row the same way
 * (normals are not renormalised), 0 keeps the first point's rows (upstream's doc says "drop"; its compaction as recalled
 * copies the columns).  A planar cloud (z = 0) gives numDiv[2] = 1, k = 0: upstream's 2-D formula.
 * order_out (the first-point index of every output point, may be NULL), out4 (4 per point) and desc_out (desc_rows per point)
 * have capacity n; *n_out = the number of voxels.  ICPMI_ERR_INVALID_ARG (last_error says why): a vsize that is not finite
 * and > 0, non-finite coordinates, numDiv[a] >= 2^24 on some axis, numDiv[0] numDiv[1] numDiv[2] > 2^32 - 1 (computed in
 * 64 bits).  n > 2^31 - 1: ICPMI_ERR_UNSUPPORTED; n == 0: nothing to do.  Entirely on the device, no float atomics: two calls
 * give the same bits (csrc/voxelgrid.hip). */
icpmi_status icpmi_voxel_grid(icpmi_handle h, const float* in4, int64_t n, const float vsize[3], int32_t average_descriptors, const float* desc,
                              int32_t desc_rows, int32_t* order_out, float* out4, float* desc_out, int64_t* n_out);

/* What icpmi_covariance_sampling worked with: the centre c, the torque normalisation L, the eigenvalues of C in ascending order and
 * the eigenvectors, column-major: basis[6 k + j] = component j of x_k (the eigenvector of eigval[k]; its sign is the solver's). */
typedef struct {
    double center[3];
    double lnorm;
    double eigval[6];
    double basis[36];
} icpmi_covsamp_info;

/* `CovarianceSamplingDataPointsFilter{nbSample, torqueNorm}` (libpointmatcher DataPointsFilters/CovarianceSampling, Gelfand et al.
 * 2003, AS RECALLED: upstream's source is not on hand).  Every quantity is double, computed from the float inputs, no contraction:
 *   1. nb_sample >= n: the cloud is returned unchanged (order_out = 0 .. n - 1, *n_out = n, info_out untouched), normals or not.
 *      Otherwise normals3 (3 per point, point-major) is required: NULL gives ICPMI_ERR_MISSING_NORMALS.
 *   2. c = the mean of x, y, z.
 *   3. L: torque_norm 0 (L1) 1; 1 (Lavg) the mean of |p_i - c|; 2 (Lmax) half the largest bounding-box extent over x, y, z.
 *      L == 0 (every point equal) uses L = 1.
 *   4. v_i = [ s tau_i ; n_i ], s = 1.0 / L, tau_i = (p_i - c) x n_i with tau_x = (a_y b_z) - (a_z b_y) and so on.
 *   5. C = sum_i v_i v_i^T; x_0 .. x_5 its eigenvectors in ASCENDING eigenvalue order.
 *   6. m_ik = v_i . x_k summed left to right over j = 0 .. 5; list k = every point sorted by the key (float)|m_ik| descending,
 *      stable (ties in ascending index order).
 *   7. t[0 .. 5] = 0; nb_sample times: k = the first index of the minimum of t; the first point of list k not yet selected is
 *      selected; t_j += m_sel,j^2 for j = 0 .. 5 in that order.
 * order_out (capacity min(n, nb_sample)) = the selected indices in selection order, *n_out = min(n, nb_sample); nb_sample == 0 gives
 * an empty cloud.  info_out (may be NULL) = the device's c, L and eigenbasis, from which the selection replays bit for bit.
 * ICPMI_ERR_INVALID_ARG (last_error says why): nb_sample < 0, torque_norm outside 0 .. 2, a planar handle (icpmi_config::is_2d:
 * upstream takes 3-D clouds only), non-finite coordinates or normals.  n > 2^31 - 1: ICPMI_ERR_UNSUPPORTED.  Entirely on the
 * device, no float atomics: two calls give the same bits (csrc/covsampling.hip). */
icpmi_status icpmi_covariance_sampling(icpmi_handle h, const float* in4, int64_t n, const float* normals3, int64_t nb_sample, int32_t torque_norm,
                                       int32_t* order_out, int64_t* n_out, icpmi_covsamp_info* info_out);

/* `NormalSpaceDataPointsFilter{nbSample 5000, seed 1, epsilon 0.09817}` (libpointmatcher DataPointsFilters/NormalSpace, Rusinkiewicz &
 * Levoy 2001, AS RECALLED: upstream's source is not on hand):
 *   1. nb_sample >= n: the cloud is returned unchanged (order_out = 0 .. n - 1, *n_out = n, bucket_out untouched), normals or not.
 *      Otherwise normals3 (3 per point, point-major) is required: NULL gives ICPMI_ERR_MISSING_NORMALS.
 *   2. The bucket of point i, from its normal (nx, ny, nz) taken as given (upstream assumes unit length):
 *        theta = (float) acos((double) clamp(nz, -1, 1));
 *        phi_d = atan2((double) ny, (double) nx), plus 2 pi (in double) when negative; phi = (float) phi_d
 *      (both go through double and are rounded once, as the angles of the DynamicPoints module: libm and the device library agree);
 *        bt = (unsigned) floorf(theta / epsilon), bp = (unsigned) floorf(phi / epsilon)              -- float32
 *        stride = (unsigned) floorf(6.2831855f / epsilon);   bucket = bt * stride + bp.
 *      This is upstream's expression, including the aliasing of a partial last phi column (bp == stride) into the next theta row.
 *      The tables hold floorf(3.14159274f / epsilon) * stride + stride + 1 buckets, the largest index the two floors can give
 *      (below 2^14 for every epsilon served).
 *   3. r_i = the (i + 1)-th value of std::minstd_rand seeded with `seed` (seeds 0 and 2147483647 are the state 1, as seed 1).  Within a
 *      bucket, points are drawn in ascending r_i (the r_i are distinct; equal ones would go in ascending index).  DEVIATION: upstream
 *      shuffles the indices with std::shuffle(std::mt19937(seed)) -- libstdc++'s own serial Fisher-Yates -- and takes from the back of
 *      each bucket; ours is a permutation any language reproduces and a device evaluates per point.
 *   4. Round-robin, in closed form: c_b = the population of bucket b, S(R) = sum_b min(c_b, R), R* = the largest R with
 *      S(R) <= nb_sample, rem = nb_sample - S(R*).  Kept: every point whose 0-based rank in its bucket is < R*, and the points of rank
 *      R* in the first `rem` buckets, in ascending bucket index, among those with c_b > R*: exactly nb_sample points.  This is
 *      upstream's loop: one point per non-empty bucket per round, in ascending bucket index, until nb_sample is reached.
 *   5. order_out (capacity min(n, nb_sample)) = the kept indices in ASCENDING order (upstream sorts its kept indices before it moves
 *      the columns), *n_out = min(n, nb_sample); nb_sample == 0 gives an empty cloud.
 * bucket_out (n entries, may be NULL) = the device's bucket of every point, from which the selection replays bit for bit.
 * ICPMI_ERR_INVALID_ARG (last_error says why): nb_sample < 0, seed < 0, epsilon outside [0.04908, 3.14159], a planar handle
 * (icpmi_config::is_2d), non-finite coordinates or normals.  n > 2^31 - 1: ICPMI_ERR_UNSUPPORTED.  Entirely on the device, no
 * atomics: two calls give the same bits (csrc/normalspace.hip). */
icpmi_status icpmi_normal_space_sampling(icpmi_handle h, const float* in4, int64_t n, const float* normals3, int64_t nb_sample, int32_t seed, float epsilon,
                                         int32_t* order_out, int64_t* n_out, int32_t* bucket_out);

/* `MaxDensityDataPointsFilter{maxDensity 10, seed 1}` (libpointmatcher DataPointsFilters/MaxDensity; the host shell's MaxDensityFilter,
 * host/DataPointsFilters.cpp, is the definition and this entry restates it bit for bit): a point in a region denser than max_density
 * survives with probability max_density / density, decided by ONE std::minstd_rand stream that only the dense points draw from.
 *   dense_i = densities[i] > max_density                       (a NaN density compares false: not dense, the point is kept)
 *   rank_i  = the number of dense points with an index below i
 *   v_i     = the (rank_i + 1)-th value of std::minstd_rand (x <- 48271 x mod 2^31 - 1) seeded with (uint32_t) seed % 2147483647, 0 taken
 *             as 1 (the engine's constructor): seeds 0, 1 and 2147483647 are the same stream, a negative seed wraps through uint32_t
 *   u_i     = (float) v_i / 2147483645.0f                      (randomSamplingMethod 0, "direct": x / float(max - min))
 *   keep[i] = dense_i ? (u_i < max_density / densities[i]) : 1 (float32, each division correctly rounded, nothing contracted; a +inf
 *             density gives the bound 0 and the point is dropped: u < 0 is false)
 * The rank is an exclusive prefix count on the device and v_i comes from a skip-ahead, so every point decides on its own: no atomics,
 * two calls give the same bits (csrc/maxdensity.hip).  max_density not finite or not > 0: ICPMI_ERR_INVALID_ARG; n == 0: ICPMI_OK;
 * n > 2^31 - 1: ICPMI_ERR_UNSUPPORTED. */
icpmi_status icpmi_max_density_keep(icpmi_handle h, const float* densities, int64_t n, float max_density, int32_t seed, uint8_t* keep);

/* `Map::updateLocalPointCloud` (Map.cpp:502-534) for a whole module chain on the RESIDENT map: the mapper modules
 * (`mapperModuleVec`, Map.cpp:506-521) and then the post filters (Map.cpp:523-525) run as one program on the device copy
 * of the map; only the scan crosses PCIe.  The device tracks the features, the `normals` and ONE scalar descriptor of
 * the map (the shipped chain's `probabilityDynamic`); for every other descriptor the host applies `src_out`:
 * new map point j was point src_out[j] of [old map (m_old points) ; scan (n points)] -- src_out[j] < m_old: an old map
 * point, else scan point src_out[j] - m_old.
 *   ICPMI_MOP_POINT_DISTANCE   f[0] = minDistNewPoint                   (PointDistanceMapperModule.cpp:28-50)
 *   ICPMI_MOP_DYNAMIC_POINTS   f[0..6] = icpmi_dynpts_params in order   (DynamicPointsMapperModule.cpp:34-172; updates the scalar)
 *   ICPMI_MOP_VOXEL            f[0] = maxSizeByNode, i = samplingMethod 0 | 1 (OctreeMapperModule.cpp:35-39: concatenate, then decimate)
 *   ICPMI_MOP_OCTREE           f[0] = maxSizeByNode, f[1] = maxPointByNode (0 = 1), i = samplingMethod 0 | 1: the octree itself
 *                              (OctreeMapperModule.cpp:8-12,35-39 -> OctreeGridDataPointsFilter: bounding-cube root, split until the
 *                              edge is <= maxSizeByNode or the node holds <= maxPointByNode points, one point per leaf, the map left
 *                              in leaf-visiting order); ICPMI_MOP_VOXEL is the fixed-lattice decimation kept for callers that want it
 *   ICPMI_MOP_SURFACE_NORMALS  i = knn, f[0] = keepDensities 0 | 1      (post filter, examples/config.yaml:26-27)
 *   ICPMI_MOP_CUT_SCALAR       f[0] = threshold, i = useLargerThan      (CutAtDescriptorThresholdDataPointsFilter, config.yaml:29-32)
 *   ICPMI_MOP_MAX_DENSITY      f[0] = maxDensity, i = seed              (post filter: icpmi_max_density_keep on the `densities` row, then
 *                              the compaction)
 * The `densities` row: a SURFACE_NORMALS step with f[0] = 1 writes it (icpmi_surface_normals_ex's densities, same pass).  Every program
 * starts without it (the scan has none, so by DataPoints::concatenate's rule the field does not survive the modules); from that step on
 * it moves with the points through every compaction of the program, it is not touched by the sensor-frame round trip, and it stays
 * resident for icpmi_get_map_densities until the next program, icpmi_set_map or append.  A MAX_DENSITY step with no such step in front
 * of it in the same program is ICPMI_ERR_INVALID_ARG ("InvalidField: MaxDensityDataPointsFilter: Error, no densities found in
 * descriptors."), checked before the program starts: the resident map is untouched.
 * The first n_modules entries are mapper modules: on a handle without a map the first one creates the map from the scan
 * (`createMap`: PointDistance / DynamicPoints take the scan as it is, Voxel decimates it) and the others update it with
 * the same scan (Map.cpp:508-516).  scan_scalar (n floats) is the scan's value of the tracked scalar, NULL if the chain
 * has none; scan_normals3 may be NULL (appended points then carry zero normals until a SURFACE_NORMALS step).
 * to_sensor = pose^-1 (sensor <- map; `pose` is the modules' argument, DynamicPointsMapperModule.cpp:51,57), from_sensor = pose.
 * With from_sensor given the post filters run exactly where the reference runs them: the whole working map is moved into the
 * sensor frame by to_sensor, filtered, and moved back by from_sensor (Map.cpp:523-525) -- every map point picks up the
 * rounding of that round trip on every update, as in the reference (two transform kernels over the map: microseconds).
 * from_sensor == NULL: post filters in the map frame, coordinates of old map points untouched (not what the reference
 * does: a replay of the bundled trajectory then leaves the reference's poses by up to 0.4 mm); to_sensor may be NULL when
 * from_sensor is and the chain has no DYNAMIC_POINTS.
 * src_capacity must be >= m_old + n_modules * n (every module appends at most the whole scan).  identity_prefix (may be NULL): when given, receives the length of the head of
 * the new map that is the untouched head of the old one (src[j] == j for j < *identity_prefix) and src_out is written
 * from that position on only -- a host that owns further descriptors leaves those rows alone and gathers the rest, and
 * an append-only chain downloads a few kilobytes instead of the whole vector. */
typedef enum {
    ICPMI_MOP_POINT_DISTANCE = 0, ICPMI_MOP_DYNAMIC_POINTS = 1, ICPMI_MOP_VOXEL = 2, ICPMI_MOP_SURFACE_NORMALS = 3, ICPMI_MOP_CUT_SCALAR = 4,
    ICPMI_MOP_OCTREE = 5, ICPMI_MOP_MAX_DENSITY = 6
} icpmi_map_op_type;
typedef struct icpmi_map_op { int32_t type; int32_t i; float f[7]; } icpmi_map_op;
icpmi_status icpmi_map_update_chain(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float* scan_scalar,
                                    const float to_sensor[16], const float from_sensor[16], const icpmi_map_op* ops, int32_t n_ops,
                                    int32_t n_modules, int32_t* src_out, int64_t src_capacity, int64_t* identity_prefix, int64_t* new_m);
/* The same on the scan staged by icpmi_register_prior, moved by `correction` first (Mapper.cpp:221). */
icpmi_status icpmi_map_update_chain_staged(icpmi_handle h, const float correction[16], const float* scan_scalar, const float to_sensor[16],
                                           const float from_sensor[16], const icpmi_map_op* ops, int32_t n_ops, int32_t n_modules,
                                           int32_t* src_out, int64_t src_capacity, int64_t* identity_prefix, int64_t* new_m);
/* The tracked scalar descriptor of the resident map: upload after a icpmi_set_map (m must equal the map size),
 * download next to icpmi_get_map (no map, or an empty resident map: ICPMI_OK and nothing written, like icpmi_get_map's 0 points). */
icpmi_status icpmi_set_map_scalar(icpmi_handle h, const float* scalar, int64_t m);
icpmi_status icpmi_get_map_scalar(icpmi_handle h, float* scalar_out, int64_t capacity);
/* The `densities` row of the resident map (see ICPMI_MOP_SURFACE_NORMALS above), one float per point in icpmi_get_map's order.  No map,
 * an empty resident map or no valid row: ICPMI_OK and nothing written. */
icpmi_status icpmi_get_map_densities(icpmi_handle h, float* densities_out, int64_t capacity);

/* Input-side filters as ONE pass (`Mapper::applyInputFilters`, Mapper.cpp:187-191: the DistanceLimit radius filter of
 * Mapper.cpp:27-31 followed by the `input:` chain, e.g. the two BoundingBox filters of examples/config.yaml:2-18): every
 * filter of these two kinds is a per-point predicate, so a run of them is one fused kernel and one compaction instead
 * of one pass + one copy of every descriptor per filter.  keep[i] = 1 iff point i passes ALL filters.
 *   ICPMI_FILT_DISTANCE_LIMIT  i = dim (-1: radial distance, 0..2: |coordinate|), f[0] = dist, f[1] = removeInside (0 | 1):
 *                              v = dim < 0 ? sqrt(x^2 + y^2 + z^2) : |p[dim]|; kept iff removeInside ? v > |dist| : v < |dist|
 *   ICPMI_FILT_BOUNDING_BOX    f[0..2] = xMin, yMin, zMin, f[3..5] = xMax, yMax, zMax, i = removeInside:
 *                              inside iff min < p < max on all three axes; kept iff removeInside ? !inside : inside */
typedef enum { ICPMI_FILT_DISTANCE_LIMIT = 0, ICPMI_FILT_BOUNDING_BOX = 1 } icpmi_point_filter_type;
typedef struct icpmi_point_filter { int32_t type; int32_t i; float f[6]; } icpmi_point_filter;
icpmi_status icpmi_filter_points(icpmi_handle h, const float* in4, int64_t n, const icpmi_point_filter* filters, int32_t n_filters,
                                 uint8_t* keep);

/* The four sensor-model DataPointsFilters of the classic mapper chain as ONE pass (libpointmatcher 1.4.x, AS RECALLED: upstream's
 * source is not on hand): each is a per-point function of the position p = (x, y, z) (the first three feature rows), the point's
 * `normals` column n and a sensor position s, so a run of them is one kernel and -- with a Shadow step -- one compaction.  The
 * program holds up to 8 steps, evaluated in order for every point; od (`observationDirections`), n, the keep flag and the noise
 * live in registers across the steps.
 *   ICPMI_SM_OBSERVATION_DIRECTION  f[0..2] = s = (x, y, z):  od = s - p                    (ObservationDirectionDataPointsFilter)
 *   ICPMI_SM_ORIENT_NORMALS         i = towardCenter (0 | 1): d = n_x od_x + n_y od_y + n_z od_z, summed left to right; n = -n when
 *                                   towardCenter ? d < 0 : d > 0                             (OrientNormalsDataPointsFilter)
 *   ICPMI_SM_SHADOW                 f[0] = eps in [0, 1]: v = | (n / |n|) . (p / |p|) |, each vector divided by its norm first, the
 *                                   three products summed left to right; kept iff v > eps.  It reads the point's own position, not
 *                                   od: upstream takes the cloud's origin for the sensor.  |n| == 0, |p| == 0 or a NaN make v NaN,
 *                                   the comparison false and the point dropped, as Eigen's normalized() does upstream
 *                                                                                            (ShadowDataPointsFilter)
 *   ICPMI_SM_SIMPLE_SENSOR_NOISE    i = sensorType, f[0] = gain (finite, > 0); dist = |p|:
 *                                     0 Sick LMS-1xx, 1 Hokuyo URG-04LX, 2 Hokuyo UTM-30LX with (minRadius, beamAngle, beamConst) =
 *                                     (0.012, 0.0068, 0.0008), (0.028, 0.0013, 0.0001), (0.018, 0.0006, 0.0015):
 *                                       t = beamAngle * dist + beamConst; noise = gain * (t > minRadius ? t : minRadius)
 *                                     3 Kinect, 4 Xtion: noise = ((gain * 0.5) * 0.00285) * (dist * dist)
 *                                   Whether upstream applies `gain` at all is recalled, not checked (SimpleSensorNoiseDataPointsFilter)
 * Arithmetic: float32 throughout, every constant rounded to float32, in exactly the order written; a squared norm is
 * x x + y y + z z summed left to right, a norm its sqrtf; products, sums, divisions and square roots are each correctly rounded and
 * never contracted (the library is compiled with -ffp-contract=off), so the results equal a float32 restatement bit for bit.
 * Inputs (host pointers): in4 (4 per point); normals3_in (3 per point, point-major) is needed by ORIENT_NORMALS and SHADOW: NULL gives
 * ICPMI_ERR_MISSING_NORMALS; obs_dir3_in (3 per point) is what an ORIENT_NORMALS step reads when no OBSERVATION_DIRECTION step comes
 * before it in the program: NULL then gives ICPMI_ERR_INVALID_ARG ("InvalidField: ... cannot find observation directions").
 * Outputs, written only when the program produces them: normals3_out (3 n) after an ORIENT_NORMALS step (required then);
 * obs_dir3_out (3 n) after an OBSERVATION_DIRECTION step (optional: NULL skips it); noise_out (n) after a SIMPLE_SENSOR_NOISE step
 * (required; the last such step wins); keep_out (n bytes, 1 = kept by every SHADOW step) after a SHADOW step (required).  Steps after
 * a SHADOW step are evaluated for dropped points too: the caller compacts every row with keep_out, which is what filtering one by
 * one gives.  A required output that is NULL, an unknown step type, more than 8 steps, eps outside [0, 1] or not finite, a sensorType
 * outside 0 .. 4, a gain that is not finite and > 0: ICPMI_ERR_INVALID_ARG.  n == 0: ICPMI_OK; n > 2^31 - 1: ICPMI_ERR_UNSUPPORTED.
 * Planar handles (icpmi_config::is_2d) are served with z == 0 and 3-row normals, as elsewhere.  One thread per point, no atomics, no
 * shared memory: two calls give the same bits (csrc/ops.hip: sensor_model_kernel). */
typedef enum { ICPMI_SM_OBSERVATION_DIRECTION = 0, ICPMI_SM_ORIENT_NORMALS = 1,
               ICPMI_SM_SHADOW = 2, ICPMI_SM_SIMPLE_SENSOR_NOISE = 3 } icpmi_sensor_step_type;
typedef struct icpmi_sensor_step { int32_t type; int32_t i; float f[4]; } icpmi_sensor_step;
icpmi_status icpmi_sensor_model(icpmi_handle h, const float* in4, int64_t n,
                                const float* normals3_in, const float* obs_dir3_in,
                                const icpmi_sensor_step* steps, int32_t n_steps,
                                float* normals3_out, float* obs_dir3_out,
                                float* noise_out, uint8_t* keep_out);

/* Sweep deskewing: per-point motion compensation of one scan.  A spinning lidar takes ~0.1 s per sweep, and the reference tells its
 * users to switch deskewing on (docs/UsingInRos.md:211-224); there it lives in the ROS wrapper, in front of applyInputFilters ->
 * processInput, because it needs tf2's interpolation.  The semantics are tf2's lookup AS RECALLED (the wrapper's source is not on
 * hand): the caller gives the sensor's motion over the sweep as K timed poses of the sensor in a fixed frame, translation p_k and unit
 * quaternion q_k at time s_k; the pose T(tau) at s_k <= tau <= s_{k+1} has its translation interpolated linearly and its rotation by
 * slerp along the shorter arc; deskewing to the time ref sends a point x_i measured at tau_i to T(ref)^-1 T(tau_i) x_i, and rows
 * that rotate with the cloud (`normals`) are rotated by the rotation part of the same transform, as icpmi_transform does.
 *
 * icpmi_deskew_table (no handle, no device call, double precision) is the preparation every call makes, exposed so that it can be
 * checked on its own: T(ref_s) is interpolated from the table; M_k = T(ref_s)^-1 T_k is formed for every k and its quaternion
 * normalised; walking k upwards, q_{k+1} is negated when q_k . q_{k+1} < 0; per segment Omega_k = 2 atan2(|q_{k+1} - q_k|,
 * |q_{k+1} + q_k|) and inv_sin_k = 1 / sin(Omega_k), or 0 when Omega_k < 2^-20 (a zero marks the segment as plain lerp); everything is
 * then rounded to float32: q4 (4 K: x y z w), p3 (3 K), omega (K - 1), inv_sin (K - 1).  The poses being relative to ref, the
 * translations are the centimetres of one sweep and not map coordinates, and the angle never comes from acosf of a number next to 1:
 * that is what makes float32 enough on the device.
 *
 * The device pass, one thread per point, no atomics (csrc/deskew.hip: deskew_kernel).  float32 unless marked, in exactly the order
 * written, every product, sum and division correctly rounded and never contracted (-ffp-contract=off), so a float32 restatement is
 * unambiguous up to sinf:
 *   tau = (double)t_rel[i] * time_unit_s                                  (fp64); a NaN raises the error flag
 *   round_s > 0:  tau = rint(tau / round_s) * round_s                     (fp64, ties to even)
 *   tau outside [s_0, s_{K-1}]:  extrapolate ? clamped to the bound : the error flag
 *   k = the largest index in [0, K - 2] with s_k <= tau  (s_k <= tau < s_{k+1}; tau == s_{K-1} belongs to the last segment, u = 1)
 *   u = (float)((tau - s_k) / (s_{k+1} - s_k))                            (fp64, rounded once);  um = 1 - u
 *   inv_sin_k == 0 ?  w0 = um, w1 = u  :  w0 = sinf(um * Omega_k) * inv_sin_k,  w1 = sinf(u * Omega_k) * inv_sin_k
 *   q = w0 q_k + w1 q_{k+1}  (per component, not renormalised, as in tf2);   p = um p_k + u p_{k+1}  (per component)
 *   xx = qx qx, yy = qy qy, zz = qz qz, xy = qx qy, xz = qx qz, yz = qy qz, wx = qw qx, wy = qw qy, wz = qw qz
 *   R = [ 1 - 2 (yy + zz), 2 (xy - wz), 2 (xz + wy) ;  2 (xy + wz), 1 - 2 (xx + zz), 2 (yz - wx) ;  2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy) ]
 *   out_r = ((R_r0 x + R_r1 y) + R_r2 z) + p_r;  the fourth component is copied through;  normal_r = (R_r0 nx + R_r1 ny) + R_r2 nz
 * in4 / out4: 4 per point; t_rel: one float per point, the point's time in units of time_unit_s from the scan's stamp (the bundled
 * scans' `t` descriptor: nanoseconds, time_unit_s = 1e-9); in_normals3 / out_normals3 (3 per point) both or neither.
 * ICPMI_ERR_INVALID_ARG with a message (icpmi_last_error(h); icpmi_last_error(NULL) after icpmi_deskew_table): a NULL pointer, n_poses
 * outside 2 .. ICPMI_DESKEW_MAX_POSES, stamps not strictly increasing, a non-finite entry, a quaternion with | |q| - 1 | > 1e-3, ref_s
 * outside [stamp_s[0], stamp_s[n_poses - 1]], time_unit_s not finite and > 0, round_s not finite and >= 0; a raised error flag (the
 * flag is one word, written with an ordinary store of the constant 1: out4 is then unspecified, and the host-pointer variant does not
 * copy it back).  n == 0: ICPMI_OK; n > 2^31 - 1: ICPMI_ERR_UNSUPPORTED.  A planar handle (icpmi_config::is_2d) takes planar motion
 * only -- tz, qx and qy of every pose exactly 0, else ICPMI_ERR_INVALID_ARG -- and such a motion keeps z = 0 exactly: the third row
 * and column of R are then exactly those of the identity.  Two calls give the same bits. */
enum { ICPMI_DESKEW_MAX_POSES = 1024 };
typedef struct icpmi_sweep_motion {
    int32_t n_poses;        /* 2 .. ICPMI_DESKEW_MAX_POSES */
    int32_t extrapolate;    /* 0: a point time outside [stamp_s[0], stamp_s[n-1]] fails the call (tf2's ExtrapolationException); 1: clamped to the span */
    const double* stamp_s;  /* n_poses, strictly increasing, seconds relative to the scan's stamp */
    const double* pose7;    /* n_poses x (tx ty tz qx qy qz qw); | |q| - 1 | <= 1e-3 */
    double ref_s;           /* the time the output is expressed at, inside the span */
    double time_unit_s;     /* seconds per unit of t_rel: 1e-9 for the bundled `t`, 1 for seconds; finite, > 0 */
    double round_s;         /* > 0: point times are rounded to the nearest multiple (rint, ties to even) first -- the wrapper's deskewing_round_to_nanosecs; 0: none */
} icpmi_sweep_motion;
icpmi_status icpmi_deskew_table(const icpmi_sweep_motion* m, float* q4, float* p3, float* omega, float* inv_sin);
icpmi_status icpmi_deskew(icpmi_handle h, const float* in4, int64_t n, const float* t_rel, const icpmi_sweep_motion* m,
                          float* out4, const float* in_normals3, float* out_normals3);
/* the same with in4 / t_rel / out4 / the normals as device pointers, on the handle's stream; out4 == d_in4 and d_out_normals3 ==
 * d_in_normals3 are allowed (a thread reads its point before it writes it).  The call waits for the error flag before it returns.
 * In place and followed by icpmi_register_prior_dev, a scan that is already in HBM is deskewed and registered without crossing PCIe. */
icpmi_status icpmi_deskew_dev(icpmi_handle h, const float* d_in4, int64_t n, const float* d_t_rel, const icpmi_sweep_motion* m,
                              float* d_out4, const float* d_in_normals3, float* d_out_normals3);

/* Sweep registration: the sensor's motion WITHIN one scan estimated by ICP, for callers that have no IMU or odometry to hand to
 * icpmi_deskew (continuous-time ICP in its simplest linear form: Dellenbach et al. 2022, CT-ICP, with two poses per sweep).  Not
 * libpointmatcher's; off unless called.  Served on a 3-D handle with ICPMI_MIN_POINT_TO_PLANE and a map with normals.
 *
 * Unknowns: the sensor's poses in the map frame at sweep begin, T_b, and at sweep end, T_e, held on the host in double as translation
 * + unit quaternion.  Point i has the time fraction
 *   alpha_i = clamp(((double)t_rel[i] * time_unit_s - begin_s) / (end_s - begin_s), 0, 1)      (fp64, rounded once to float32)
 * kept in a device row in the caller's order; a NaN time is ICPMI_ERR_INVALID_ARG.  One iteration:
 *  1. deskew: deskew_kernel as icpmi_deskew_dev runs it, out of place, with the table of the motion {stamps begin_s, end_s; poses T_b,
 *     T_e; ref_s = end_s; extrapolate = 1; round_s = 0}: the work buffer holds the scan as seen from the end pose.  With T_b == T_e the
 *     table is exactly the identity (q = (0, 0, 0, 1), p = 0) and the work buffer equals the scan bit for bit.
 *  2. match and select: the front of icpmi_residual_error_dev for the work buffer under T_e -- centring and tile sort, the pose in the
 *     centred frame formed in double as [R | t + R mu - mu] (mu = icpmi_get_map_mean), the matcher's launch and the chain's outlier
 *     filters as a registration's first iteration runs them.
 *  3. pair sums (csrc/sweep.hip: sweep_pairs_kernel).  Per pair with weight w != 0, in float32 exactly as the point-to-plane pair sums
 *     form them: p = the reading's point under the centred pose, q = its match, n = the match's normal,
 *       F = [p.y n.z - p.z n.y, p.z n.x - p.x n.z, p.x n.y - p.y n.x, n.x, n.y, n.z],   r = (p.x - q.x) n.x + (p.y - q.y) n.y + (p.z - q.z) n.z
 *     and a = alpha[original index of the reading's point].  In double: wf_i = (double)w * F_i, m_ij = wf_i * F_j (i <= j), gr_i = wf_i * r,
 *       M0_ij += m_ij,  M1_ij += a m_ij,  M2_ij += (a a) m_ij,   g0_i += gr_i,  g1_i += a gr_i,   sum w,  pairs += 1,  sum w r^2 += ((double)w * r) * r
 *     sums[80]: [0..20] M0, upper triangle row-major ((0,0) .. (0,5), (1,1) .. (5,5)); [21..41] M1; [42..62] M2; [63..68] g0; [69..74]
 *     g1; [75] sum w; [76] pairs; [77] sum w r^2; [78], [79] zero.  (icpmi_minimize_step's sums hold b = -g0 at [21..26].)
 *     No atomics: 256 workgroups walk the n * knn slots with a grid stride, each reduces its threads' sums in a fixed butterfly and
 *     writes one row of partials; one workgroup of 640 threads then adds the rows: value v is the sum over c = 0 .. 7, in that order,
 *     of the sums over i = 0 .. 31, in that order, of row c + 8 i.  Two calls give the same bits.
 *  4. the 80 doubles, the state's error word and the quantile filter's limit come back in one copy.
 *  5. the step, on the host in double (icpmi_sweep_solve): x = (xi_b, xi_e), each (omega, t), for the model in which point i moves by
 *     omega(a) x p + t(a) with (omega(a), t(a)) = (1 - a) xi_b + a xi_e:
 *       A = [[M0 - 2 M1 + M2, M1 - M2], [M1 - M2, M2]],   rhs = -[g0 - g1 ; g1]
 *     Motion prior (lambda_rot, lambda_trans >= 0): L = (sum w) diag(lambda_rot x 3, lambda_trans x 3), D = [-I I]; A += D^T L D, rhs -=
 *     D^T L d, where d is the sum of xi_e - xi_b over the call's earlier iterations: a first-order pull of the relative motion towards
 *     the one the caller's two priors have.  The system is factored in the variables (xi_b, delta = xi_e - xi_b), a congruence with unit
 *     determinant under which it reads [[M0, M1], [M1, M2 + L]] (xi_b ; delta) = [-g0 ; -g1 - L d] -- the prior sits in one block, so large
 *     weights cancel nothing -- by Cholesky; a pivot <= 1e-12 x the largest diagonal entry is ICPMI_ERR_NAN ("the motion within the sweep
 *     is not observable: a prior weight is needed"); pairs == 0 is ICPMI_ERR_NO_POINT_TO_MINIMIZE.  xi_e = xi_b + delta.
 *     Each step becomes a rigid transform as the loop's steps do -- the rotation exp([omega]x), the translation t as it is -- moves from
 *     the centred frame to the map frame, S = [R_s | t + mu - R_s mu], and T_b <- S(xi_b) T_b, T_e <- S(xi_e) T_e (quaternions renormalised).
 *  6. stop: after max_iterations (ICPMI_STOP_COUNTER), or as soon as both steps have |omega| < min_step_rot and |t| < min_step_trans
 *     (ICPMI_STOP_DIFFERENTIAL; the steps of that iteration are applied).
 * out4 (may be NULL): the scan deskewed to the end pose, in the sensor frame, under the final motion -- one more launch of step 1;
 * icpmi_deskew with stamps {begin_s, end_s}, poses result->pose7, ref_s = end_s, extrapolate = 1 gives the same bits.
 * ICPMI_ERR_INVALID_ARG with a message: a NULL pointer, force_4dof, force_2d, is_2d, covariance or a non-zero degeneracy_threshold in
 * the handle's config, another minimiser, no map, a prior that is not rigid (the check of icpmi_residual_error), begin_s >= end_s, a
 * non-finite option, a negative prior weight, a NaN point time.  ICPMI_ERR_MISSING_NORMALS: a map without normals.  Outlier filters whose
 * answer is iteration state are refused as icpmi_residual_error refuses them.  n == 0: ICPMI_OK with the priors.  A later registration
 * on the handle returns the bits it would have returned without the sweep call; the covariance and the localizability report of the
 * registration before it are dropped. */
typedef struct icpmi_sweep_options {
    double begin_s, end_s;   /* the sweep's span, seconds relative to the scan's stamp; begin_s < end_s */
    double time_unit_s;      /* seconds per unit of t_rel (icpmi_sweep_motion::time_unit_s); finite, > 0 */
    int32_t max_iterations;  /* >= 1; icpmi_sweep_options_default: 12 */
    float min_step_rot;      /* rad; < 0: the chain's min_diff_rot */
    float min_step_trans;    /* m; < 0: the chain's min_diff_trans */
    int32_t pad;
    double lambda_rot;       /* prior weights, >= 0; icpmi_sweep_options_default: 0 */
    double lambda_trans;
    int32_t reserved[8];     /* zero */
} icpmi_sweep_options;
typedef struct icpmi_sweep_result {
    float T_begin[16], T_end[16]; /* column-major 4 x 4, map frame */
    double pose7[14];             /* the same two poses in double: tx ty tz qx qy qz qw of begin, then of end */
    int32_t iterations;           /* iterations run (icpmi_sweep_sums: 0) */
    int32_t stop_reason;          /* ICPMI_STOP_COUNTER or ICPMI_STOP_DIFFERENTIAL */
    int64_t pairs;                /* the rest: of the last iteration's pair sums */
    double weight_sum;
    double sum_sq;                /* sum w r^2 */
    float weighted_point_used_ratio;
    float trimmed_limit;          /* -1 without a quantile filter */
    int32_t reserved[8];
} icpmi_sweep_result;
void icpmi_sweep_options_default(icpmi_sweep_options* opts); /* span 0 .. 0.1 s, time_unit_s 1e-9, 12 iterations, the chain's thresholds, no prior */
icpmi_status icpmi_register_sweep(icpmi_handle h, const float* scan4, int64_t n, const float* t_rel, const float prior_begin16[16],
                                  const float prior_end16[16], const icpmi_sweep_options* opts, icpmi_sweep_result* result, float* out4);
/* the same with scan4 / t_rel / out4 as device pointers, on the handle's stream; d_out4 must not be d_scan4 */
icpmi_status icpmi_register_sweep_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_t_rel, const float prior_begin16[16],
                                      const float prior_end16[16], const icpmi_sweep_options* opts, icpmi_sweep_result* result, float* d_out4);
/* the stage call (the analogue of icpmi_minimize_step): steps 1 to 4 once under the given poses; stats (may be NULL): the poses as
 * given and the figures of that pass.  n >= 1. */
icpmi_status icpmi_sweep_sums(icpmi_handle h, const float* scan4, int64_t n, const float* t_rel, const float T_begin16[16],
                              const float T_end16[16], const icpmi_sweep_options* opts, double sums80[80], icpmi_sweep_result* stats);
/* step 5's system alone: no handle, no device call (messages: icpmi_last_error(NULL)).  d6: NULL = zero.  x12 = (xi_b, xi_e). */
icpmi_status icpmi_sweep_solve(const double sums80[80], double lambda_rot, double lambda_trans, const double d6[6], double x12[12]);

/* `Map::unloadCells` binning (Map.cpp:206-209,232-235): ijk3[3 i + r] = floor(p_r / cell_size). */
icpmi_status icpmi_bin_cells(icpmi_handle h, const float* pts4, int64_t n, float cell_size, int32_t* ijk3);

/* ---- multi-GPU: scan-sharded mapping (BASELINE config 5) ----
 * One process and one handle per GPU, the map replicated, every rank registering its own scan stream; the one exchange is map
 * growth: the points every rank accepted are all-gathered over RCCL (xGMI) so that all replicas append the same set -- what a
 * host then bins into 20 m cells for its CellManager (Map.cpp:206-229).  No reference analogue (the reference is one process).
 *   icpmi_comm_get_unique_id  rank 0 creates the id (an ncclUniqueId); the application hands it to the other ranks
 *   icpmi_comm_init           collective over all ranks: ncclCommInitRank on the handle's device
 *   icpmi_staged_merge_allgather  one map-growth epoch, entirely on the device: the scan staged by icpmi_register_prior is moved
 *       by `correction` (Mapper.cpp:221); the points at least min_dist from the resident map are compacted
 *       (PointDistanceMapperModule.cpp:33-42); counts, then the padded point blocks, are all-gathered on the handle's stream;
 *       the blocks are merged in rank order, block r keeping only the points that are at least min_dist from the points
 *       accepted from ranks < r (exactly what one mapper would have appended had it processed the scans in rank order);
 *       the merged set is appended to the resident map, its normals recomputed (normals_knn > 0) and the index rebuilt.
 *       No accepted point crosses PCIe unless merged_out4 (capacity merged_capacity points) asks for the merged set.
 *       Without a communicator the handle is its own single rank.
 *       Collective discipline (v3): the call is a collective -- EVERY rank of the communicator must make it once per epoch, also a
 *       rank that has nothing to add: `correction == NULL` (or nothing staged, see icpmi_stage_discard) contributes zero points and
 *       still receives and appends what the others accepted.  A rank whose local part fails reports count -1 and ALL ranks return an
 *       error together without appending; buffers are grown to the gathered sizes behind a second one-word exchange, so no rank can
 *       leave between two collectives.  The merged set is always appended: when merged_capacity is smaller than the merged set,
 *       merged_out4 receives the first merged_capacity points, *merged_n the full count, the status stays ICPMI_OK and
 *       icpmi_staged_merged_points returns the whole set -- replicas never diverge over a host buffer.
 *   icpmi_staged_merged_points  the merged set of the last epoch (out4 == NULL: only *n), kept on the device until the next epoch
 *   icpmi_staged_bin_cells (r6)  the merged set of the last epoch binned into cubic cells of edge cell_size ON THE DEVICE -- Map.cpp:206-229's
 *       per-point loop (cell = floor(coordinate / cell_size) per axis, Map.cpp:472-480) feeding RAMCellManager.cpp:13-16 -- and appended,
 *       cell after cell (cells in the order of their first point, the points of a cell in merged order: what Map::binIntoCells yields on
 *       the host), to the handle's device-resident CELL LOG.  Returned per cell r < *n_cells: ijk3[3 r ..], counts[r] and offsets[r], the
 *       position of the cell's run in the log.  Only this table crosses PCIe.  Once per epoch (a second call for the same epoch is an
 *       ICPMI_ERR_INVALID_ARG); capacity < *n_cells: ICPMI_ERR_INVALID_ARG with *n_cells set and nothing appended; more than 4096 cells
 *       touched by one epoch: ICPMI_ERR_UNSUPPORTED (fetch icpmi_staged_merged_points and bin on the host).
 *   icpmi_cell_log_configure     cell_size > 0: from now on every epoch enqueues that binning itself, between its merge and its append (the kernels
 *                                run in the shadow of the index insert); icpmi_staged_bin_cells with the same cell_size then only collects the
 *                                table.  0: off (the default)
 *   icpmi_cell_log_read          `count` points of the log from `offset` (out4 == NULL: only *log_size, the points in the log)
 *   icpmi_cell_log_clear         forgets the log (CellManager::clearAllCells)
 *   icpmi_stage_discard          drops the scan staged by icpmi_register_prior (e.g. after its registration failed: the rank then
 *                                takes part in the epoch empty-handed and reports its own error afterwards) */
typedef struct icpmi_comm_id { char bytes[128]; } icpmi_comm_id;
icpmi_status icpmi_comm_get_unique_id(icpmi_comm_id* id);
icpmi_status icpmi_comm_init(icpmi_handle h, const icpmi_comm_id* id, int32_t n_ranks, int32_t rank);
icpmi_status icpmi_comm_destroy(icpmi_handle h);
/* What the handle's communicator reports about itself (RCCL: ncclCommCount / ncclCommUserRank); kind 0 = none (the handle is its own
 * single rank), 1 = RCCL, 2 = the loopback test communicator.  Any pointer may be NULL. */
icpmi_status icpmi_comm_info(icpmi_handle h, int32_t* n_ranks, int32_t* rank, int32_t* kind);
icpmi_status icpmi_staged_merge_allgather(icpmi_handle h, const float correction[16], float min_dist, int32_t normals_knn,
                                          int64_t* accepted_local, int64_t* appended_total, int64_t* new_m, float* merged_out4,
                                          int64_t merged_capacity, int64_t* merged_n);
icpmi_status icpmi_staged_merged_points(icpmi_handle h, float* out4, int64_t capacity, int64_t* n);
icpmi_status icpmi_staged_bin_cells(icpmi_handle h, float cell_size, int32_t* ijk3, int64_t* offsets, int64_t* counts, int64_t capacity,
                                    int64_t* n_cells);
icpmi_status icpmi_cell_log_configure(icpmi_handle h, float cell_size);
icpmi_status icpmi_cell_log_read(icpmi_handle h, int64_t offset, int64_t count, float* out4, int64_t* log_size);
icpmi_status icpmi_cell_log_clear(icpmi_handle h);
icpmi_status icpmi_stage_discard(icpmi_handle h);

/* ---- plumbing ---- */
/* Use an externally owned hipStream_t (e.g. torch's current stream) instead of the handle's own. */
icpmi_status icpmi_set_stream(icpmi_handle h, void* hip_stream);
/* Grid parameters chosen by the last set_map: cell edge, dims[3], number of cells (for DESIGN/bench). */
icpmi_status icpmi_get_grid_info(icpmi_handle h, float* cell, int32_t dims[3], int64_t* n_cells, int64_t* n_occupied);
int32_t      icpmi_version(void);
/* "icpmi <version> src:<stamp>": <stamp> = the first 16 hex digits of the SHA-256 over the library's sources (csrc Makefile: sorted *.hip, common.h,
 * solve.h, include/icpmi.h) as they were when this binary was linked -- tests/conftest.py recomputes it from the tree and refuses to run GPU
 * tests against a binary built from other sources. */
const char*  icpmi_build_info(void);
/* The library caches freed device blocks per device (at most ICPMI_ALLOC_CACHE_MB, default 1024) so that a mapper that is dropped and rebuilt
 * finds its ~300 arrays again.  A host that shares the GPU with another allocator calls this when it is done with a mapper: every cached
 * block goes back to the runtime now; live handles stay valid. */
icpmi_status icpmi_trim_cache(void);
/* Diagnostics of the last registration (engine internals, not part of the reference surface).  Slots 10 / 11: k = 1 loop of a single
   reading -- queries the matcher's helper workgroups ran in place of their home workgroup, summed over the launches / far-seeded queries that
   found their launch's defer list full and stayed at home (both 0 under ICPMI_NN_DEFER=0, in a batch and for k > 1).  Slots 12 / 13 (r5): iterations of a k > 1 loop whose
   quantile selection took its level 0 from the NN kernel's window / from the full histogram behind a window that missed.
   Slot 23: normals an append-only update recomputed whose copy in the registration index was not found, hence not rewritten, since the handle
   was created -- 0 on a sound handle (read back from the device: the call waits for the handle's stream). */
icpmi_status icpmi_debug_counters(icpmi_handle h, uint64_t out[24]);
/* Test seam: the normals the registration index holds, by ORIGINAL index (the order of icpmi_get_map).  sorted3 (m x 3): the sorted copy the
 * k = 1 pair sums, the covariance and the voxel tables read; pn3 (m x 3, may be NULL): the copy interleaved with the points that the k > 1
 * pair sums read, written only where the handle keeps one -- *has_pn (may be NULL) says whether it does.  Both are gathered on the host
 * through the original index each level-0 position carries.  m must be the indexed map's size.  Reads only: no launch, the handle and its
 * cached loop graphs stay as they are.  ICPMI_ERR_UNSUPPORTED when the index holds no normals; ICPMI_ERR_HIP when the positions' original
 * indices are not a permutation of 0 .. m - 1 or the two copies disagree on them.  No production path calls it. */
icpmi_status icpmi_debug_index_normals(icpmi_handle h, int64_t m, float* sorted3, float* pn3, int32_t* has_pn);
/* Test seam: the matches of the last COUNTED iteration of the last single registration (icpmi_register*) on this handle, in the caller's point
 * order: row i holds the k matches of reading point i as ORIGINAL map indices, ascending by (d2, index), unfilled slots -1 / +inf; d2 as the
 * matcher computed it, against the centred map.  T_used (column-major) is the centred-frame pose that iteration's NN launch moved the centred
 * reading by, i.e. the query of point i was T_used * (p_i - mean).  n / k must be the registration's.  ICPMI_ERR_UNSUPPORTED when there is
 * nothing to read: no registration yet, one that failed, a batch (icpmi_register_batch_dev), or any other call that reused the matcher's
 * buffers or changed the map after it. */
icpmi_status icpmi_debug_last_matches(icpmi_handle h, int64_t n, int32_t k, int32_t* ids, float* d2, float T_used[16]);
/* Test seam: the self k-NN search behind icpmi_surface_normals*, and nothing else -- the same private search handle, so the cell-edge tuner's
 * history is shared with the filter.  ids (m x k, row i = the neighbours of point i) are ORIGINAL indices, laid out and converted as
 * matched_ids of icpmi_surface_normals_ex2, ascending by (d2, index); d2 (m x k) as the search kernels computed it; unfilled slots -1 / +inf.
 * info (may be NULL) describes the grid the call built: [0] the bits of the A-cell edge (float32), [1 .. 3] A-cells per axis, [4] entries of
 * the block table T, [5] queries the cell kernel queued for the level kernel, [6] builds the tuner ran, [7] 0.  No production path calls it. */
icpmi_status icpmi_debug_self_knn(icpmi_handle h, const float* pts4, int64_t m, int32_t k, int32_t* ids, float* d2, uint64_t info[8]);
/* Test seam: the squared distance of every resident point's k-th neighbour (itself counted) as the SurfaceNormal pass of the last append-only
 * update remembered it -- the state the next append's subset search selects from; +inf where fewer than k points exist.  m must be the
 * resident map's size; *knn_out (may be NULL) = that pass's knn.  ICPMI_ERR_UNSUPPORTED unless the row describes the resident map as it is
 * (a tracked pass ran and nothing rewrote the map since).  No production path calls it. */
icpmi_status icpmi_debug_resident_kth_d2(icpmi_handle h, int64_t m, float* out, int32_t* knn_out);
/* Test seam: the rank-ordered merge of icpmi_staged_merge_allgather, and nothing else, on blocks the caller hands in -- no map, no
 * communicator, nothing appended.  pts4 holds the n_ranks blocks back to back, unpadded (sum(counts) points, x y z w); the call lays block r
 * at r * stride of a device buffer of stride * n_ranks points whose padding stays uninitialised, as a gathered buffer's is, and runs the
 * epoch's merge on it.  mode 0: the epoch's own choice between the single launch and the per-block launches; 1: the per-block launches.
 * merged_out4 gets what fits in `capacity` points, *merged_n always the full count; kept_out (may be NULL) one byte per input point in input
 * order; *path_out 0 when nothing had to be decided (one non-empty block, or min_dist <= 0), 1 for the single launch, 2 for the per-block
 * launches.  ICPMI_ERR_INVALID_ARG (the message names the argument): n_ranks outside 1 .. 256, a negative count, a count above stride, a null
 * pointer where points exist; the merge's own refusals (2^31 span, 2^29 points) are ICPMI_ERR_UNSUPPORTED.  No production path calls it. */
icpmi_status icpmi_debug_merge_blocks(icpmi_handle h, const float* pts4, const int64_t* counts, int32_t n_ranks, int64_t stride, float min_dist, int32_t mode,
                                      float* merged_out4, int64_t capacity, int64_t* merged_n, uint8_t* kept_out, int32_t* path_out);
/* Test seam: the pair sums of the last COUNTED iteration of the last single registration, as its solve read them.  Off by default:
 * icpmi_debug_keep_sums(h, 1) gives the handle a block of 32 doubles that every later single registration's solve writes (the cached loop
 * graphs are dropped; batches never write it), icpmi_debug_keep_sums(h, 0) takes it away again.  Layout of sums[32] (double), as
 * icpmi_minimize_step: point-to-plane -> A (upper 21, row-major packed) then b (6); point-to-point -> sum w, sum w p (3), sum w q (3),
 * sum w q p^T (9); always [27] = sum w, [28] = number of pairs with w != 0; force2D -> [29..31] = b of the 2-D residual.  limits
 * (8 floats, slot f = filter f of the chain: Trimmed / Median / VarTrimmed), robust_scale (RobustOutlierFilter's scale) and
 * vt_ratio (the ratio VarTrimmedDist picked, -1 without one) are that iteration's; each may be NULL.  ICPMI_ERR_UNSUPPORTED when the sums
 * are not kept, or under icpmi_debug_last_matches' condition: nothing of a single registration to read. */
icpmi_status icpmi_debug_keep_sums(icpmi_handle h, int32_t on);
icpmi_status icpmi_debug_last_sums(icpmi_handle h, double sums[32], float limits[8], float* robust_scale, float* vt_ratio);

/* `errorMinimizer->getCovariance()` of PointToPlaneWithCovErrorMinimizer (upstream's formulation as recalled; Censi's closed form).
 * Needs icpmi_config::covariance = 1 (point-to-plane, 3-D clouds; force2D / force4DOF do not change the formula).  The pairs are those
 * of the LAST COUNTED iteration of the last single registration: error elements e = (query i, slot j) with weight w_e > 0 -- the weight
 * only decides whether a pair is in, its value is not used.  Everything is in the centred frame (the map minus its mean mu), as upstream's:
 *   p = T_prev (p_i - mu)   the query exactly as that iteration's NN launch formed it (T_prev = icpmi_debug_last_matches' T_used)
 *   q = m_s - mu, n = the map normal of s as stored
 *   r = |p|, d = p / r, rho = |q|, u = q / rho          (ranges measured from the map centroid, as upstream does)
 *   T_s = T_iter T_prev^-1 (the last step; T_prev^-1 = [R^T | -R^T t]), beta = -asin(T_s[2,0]), alpha = atan2(T_s[2,1], T_s[2,2]),
 *     gamma = atan2(T_s[1,0] / cos beta, T_s[0,0] / cos beta), t = T_s[0:3, 3]
 *   c = d x n, L = [[1, -gamma, beta], [gamma, 1, -alpha], [-beta, alpha, 1]]
 *   E = n . (L p + t - q),  N_r = n . (L d),  N_q = -n . u
 *   h = (n, r c),  a = (n N_r, c (E + r N_r)),  b = (n N_q, r c N_q)
 *   H = sum h h^T,  S = sum (a a^T + b b^T),  Cov = sigma^2 H^-1 S H^-1   (sigma = sensor_std_dev)
 * a / b are the derivatives of the gradient of the linearised cost sum E^2 by the reading range r and the reference range rho (the
 * factors 2 cancel).  Parameter order (tx, ty, tz, alpha, beta, gamma); `cov` is float, 6 x 6, column-major (PM::Matrix), exactly
 * symmetric.  The sums run in double on the device, per workgroup and then in a fixed order: no float atomics, two identical calls
 * give the same bits.  H not positive definite (a double Cholesky meets a pivot <= 0): Cov = FLT_MAX I, upstream's "cannot estimate".
 * A pair at zero range gives NaN, as upstream.  ICPMI_ERR_UNSUPPORTED when there is nothing to read: covariance not asked for, no
 * registration yet, one that failed, a batch (icpmi_register_batch_dev), or any other call that reused the matcher's buffers or changed
 * the map after it -- the same rule as icpmi_debug_last_matches. */
icpmi_status icpmi_get_covariance(icpmi_handle h, float cov[36]);

/* Localizability of the point-to-plane system (Zhang & Singh's solution remapping as LOAM / LeGO-LOAM / LIO-SAM carry it; NOT a
 * libpointmatcher feature).  Needs icpmi_config::degeneracy_threshold != 0 (point-to-plane, 3-D clouds, 6-DOF or force_4dof).  For one
 * iteration, from its pair sums A (6 x 6), b (6), W = sum w in double, unknown x = (omega, t):
 *   c0 = mean of the reading (centred map frame, before any pose), L = mean |p - c0| over the reading (1 when 0): one reduction per
 *        registration, both rigid-invariant; c = T c0 with T the pose the iteration's pairs were formed under
 *   1. pivot    K = [[I, -[c]x], [0, I]]:  A_c = K A K^T, b_c = K b   (rows of F become [(p - c) x n; n], unknown (omega, t + omega x c))
 *   2. scale    S = diag(1/L, 1/L, 1/L, 1, 1, 1):  A_s = S A_c S, b_s = S b_c
 *   3. decompose  force_4dof: the {2, 3, 4, 5} sub-system (n = 4), else n = 6; eigenpairs (lambda_e, v_e) of A_s ascending (double Jacobi),
 *                 mu_e = lambda_e / W -- dimensionless, independent of where the map's centroid lies; for a translation it is the share
 *                 of the pair weight that constrains the direction
 *   4. classify   direction e is degenerate when mu_e <= |threshold| or lambda_e <= n eps_f lambda_max (the solver's rank rule)
 *   5. step (threshold > 0 only)  y = sum over the non-degenerate e of v_e (v_e . b_s) / lambda_e;  omega = y_omega / L,
 *                 t = y_t - omega x c;  x is rounded to float once and goes on as the Cholesky's x does.  No direction left: x = 0.
 * The call reports the LAST COUNTED iteration of the last single registration (icpmi_register*, every variant; icpmi_minimize_step too).
 * A column of `basis` is a twist in the pivoted, scaled coordinates: turn it into a physical one as rotation omega' / lnorm about `pivot`,
 * translation as is.  ICPMI_ERR_UNSUPPORTED when there is nothing to read: the option is off, no registration yet, one that failed, a
 * batch / multistart call came after it, or the map (icpmi_set_map*, any map update), the chain (icpmi_set_config) or the stream changed
 * after it -- read the report before the map update that follows the registration, as icpmi_get_covariance.  Two identical calls give the same bits (no atomics anywhere in it). */
typedef struct {
    int32_t n;               /* 6, or 4 (force_4dof: yaw + translation)                                                              */
    int32_t n_degenerate;    /* number of degenerate directions                                                                      */
    int32_t degenerate[6];   /* flag per direction e (ascending eigenvalue); entries >= n are 0                                       */
    double  eigval[6];       /* mu_e, ascending; entries >= n are 0                                                                  */
    double  basis[36];       /* column-major: basis[6 e + i] = component i of v_e in (omega' (3), t' (3)); force_4dof: components 0, 1 */
                             /* and columns 4, 5 are 0; the sign is the solver's                                                      */
    double  pivot[3];        /* c in the map frame (the caller's frame: the map mean added back)                                     */
    double  lnorm;           /* L                                                                                                    */
    double  weight_sum;      /* W                                                                                                    */
    int64_t pairs;           /* pairs with w != 0 of that iteration                                                                  */
    int32_t iterations;      /* the iteration the report is for (1 = the first)                                                      */
    int32_t reserved[3];
} icpmi_localizability;
icpmi_status icpmi_get_localizability(icpmi_handle h, icpmi_localizability* out);

/* `errorMinimizer->getResidualError(filteredReading, filteredReference, outlierWeights, matches)` under a GIVEN pose: how well a reading
 * fits the handle's map (upstream's formulation as recalled, not checked against upstream's source).  One matcher pass, one pass of the chain's
 * outlier filters and one reduction, all on the device; a call of its own, no registration needed before it and none changed by it.
 *   1. every reading point is moved by T and matched against the map with the chain's matcher (knn, maxDist or the armed maxDistField row,
 *      epsilon / epsilon_approx): the search the first iteration of icpmi_register would run from T.
 *   2. the chain's outlier filters weigh those matches.  An ERROR ELEMENT is a pair whose match is filled and whose weight is != 0
 *      (upstream's getMatchedPoints).  A soft weight (GenericDescriptor, Robust) counts as one pair like any other: the weight decides
 *      whether a pair is in, it does not scale the residual.
 *   3. per pair, in float32, p = the moved reading point, q = the matched map point, n = its normal, d = p - q:
 *        point-to-point:  r = sqrtf(d2), d2 the matcher's squared distance of the pair (upstream sums the norms of the deltas)
 *        point-to-plane:  r = |dx nx + dy ny + dz nz| (plain multiplies and adds in that order, no fused multiply-add);
 *                         force_2d / is_2d: the x and y terms only (upstream's forcedDim)
 *   4. sum_abs = sum of r over the error elements, in double: getResidualError().  The same reduction returns sum_sq = sum r^2,
 *      max_abs = max r, pairs = the number of error elements P, weight_sum = sum w and weighted_point_used_ratio = sum w / (knn n):
 *      getOverlap() under the evaluated pose.  trimmed_limit as icpmi_stats.  kind = what was computed (1 or 2).
 *   5. P == 0: ICPMI_ERR_NO_POINT_TO_MINIMIZE (upstream's ConvergenceError); a Trimmed / Median filter that finds no filled match:
 *      ICPMI_ERR_NO_OUTLIER_TO_FILTER, as in a registration.
 * The sums run per workgroup and then in a fixed order, without atomics: two identical calls give the same bits.
 * scan4 / T mean what they mean for icpmi_register: the reading is already moved by the prior, T (column-major, NULL = identity) is a
 * correction in the map frame -- icpmi_residual_error(scan, T_out of icpmi_register(scan)) scores the registration just made.  The matcher
 * works in the centred frame (the map minus its mean mu): it moves p - mu by [R | t + R mu - mu], that translation formed in double and
 * rounded to float.  |1 - det R| > 1e-3: ICPMI_ERR_INVALID_ARG, as icpmi_transform.
 * kind: ICPMI_RES_CHAIN takes it from the handle's minimizer (IdentityErrorMinimizer: ICPMI_ERR_UNSUPPORTED -- upstream's base class has no
 * residual); ICPMI_RES_POINT_TO_PLANE without map normals: ICPMI_ERR_MISSING_NORMALS.  No map: ICPMI_ERR_INVALID_ARG.
 * Every outlier filter of the chain is served.  SurfaceNormalOutlierFilter needs scan_normals3 (rotated by T, as the loop does) and map
 * normals, else ICPMI_ERR_MISSING_NORMALS.  The rows armed by icpmi_set_reading_scalar / icpmi_set_reading_max_dist /
 * icpmi_set_reading_sensor_noise are consumed as a registration consumes them (the noise row is not read).  A filter whose answer is state
 * of a registration's iterations -- RobustOutlierFilter with scaleEstimator berg, or with nbIterationForScale > 0 -- is
 * ICPMI_ERR_UNSUPPORTED: it is not served with a guess.
 * _dev: the reading (and its normals) in HBM.  _staged: the scan icpmi_register_prior* left in HBM (the stage icpmi_map_update_staged
 * consumes; no upload), ICPMI_ERR_INVALID_ARG without one.
 * Afterwards icpmi_get_covariance still returns the covariance of the registration before the call; icpmi_debug_last_matches and
 * icpmi_debug_last_sums have nothing to read (the matcher's buffers were reused), as after icpmi_knn. */
typedef struct {
    double  sum_abs;   /* getResidualError() */
    double  sum_sq;
    float   max_abs;
    float   weighted_point_used_ratio;
    double  weight_sum;
    int64_t pairs;
    float   trimmed_limit;   /* as icpmi_stats */
    int32_t kind;            /* what was computed: 1 or 2 */
    int32_t reserved[4];
} icpmi_residual;

typedef enum {
    ICPMI_RES_CHAIN = 0,
    ICPMI_RES_POINT_TO_POINT = 1,
    ICPMI_RES_POINT_TO_PLANE = 2
} icpmi_residual_kind;

icpmi_status icpmi_residual_error(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float T[16],
                                  int32_t kind, icpmi_residual* out);
icpmi_status icpmi_residual_error_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, const float T[16],
                                      int32_t kind, icpmi_residual* out);
icpmi_status icpmi_residual_error_staged(icpmi_handle h, const float T[16], int32_t kind, icpmi_residual* out);

/* The same reading under MANY poses in one call: what ranks the start poses of a relocalisation.  T holds n_poses (1 .. 4096) matrices of
 * 16 floats, column-major; out[p] and status[p] are, bit for bit (the doubles too), what
 *     icpmi_residual_error_dev(h, d_scan4, n, d_scan_normals3, T + 16 p, kind, &out[p])
 * returns on the same handle, whichever poses share a launch and in whatever order they come.
 *   Errors of the whole call are the return value, found before anything is enqueued, with the codes of the single call: no map, NULL
 *   arguments, a bad kind, n_poses out of range, n == 0 (the convergence error of an empty reading), missing normals, the refused Robust
 *   filters, IdentityErrorMinimizer under ICPMI_RES_CHAIN, a missing one-shot row.  out and status are then all zero.
 *   Errors of one pose go to status[p]: a T[p] that is not rigid (ICPMI_ERR_INVALID_ARG; that pose is not launched),
 *   ICPMI_ERR_NO_OUTLIER_TO_FILTER, ICPMI_ERR_NO_POINT_TO_MINIMIZE.  status == NULL: the first of them is the return value, as in
 *   icpmi_register_batch_dev.
 * The rows armed by icpmi_set_reading_scalar / icpmi_set_reading_max_dist belong to the reading: the call consumes them once and every pose
 * uses them.  The reading is centred and tile-sorted once per call.
 * The chains icpmi_register_batch_dev runs together (knn 1 on the grid pyramid, a finite maxDist below the top level's cell, at most one
 * Trimmed / Median filter, no filter that reads descriptors, no maxDistField row) go in chunks of up to 16 poses: per chunk one matcher
 * launch, one selection and the two reduction kernels of the single call with one slice, one loop state and one set of histograms per
 * pose, the chunks back to back on the handle's stream, and ONE read-back of the n_poses results at the end.  Every other chain runs pose
 * after pose through the single call's path on the prepared reading.  *batched (may be NULL) = the poses that took the batched launches
 * (the rigid ones, or 0).
 * Afterwards the handle is as after icpmi_residual_error.  The variant without _dev takes the reading (and its normals) from the host and
 * uploads them once. */
icpmi_status icpmi_residual_error_poses_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, const float* T,
                                            int32_t n_poses, int32_t kind, icpmi_residual* out, icpmi_status* status, int32_t* batched);
icpmi_status icpmi_residual_error_poses(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float* T,
                                        int32_t n_poses, int32_t kind, icpmi_residual* out, icpmi_status* status, int32_t* batched);

/* One sensor-frame scan in HBM registered from n_starts (1 .. 16) priors at once: the scan is moved by every prior on the device
 * (the transform of icpmi_register_prior_dev) into slices of its own and the slices go through icpmi_register_batch_dev's loop
 * (fixed_iterations as there; a chain the batch does not serve registers them one after the other).  T_out + 16 s, stats[s] and status[s]
 * are bit for bit what icpmi_register_prior_dev(h, d_scan4, n, priors + 16 s, ...) returns alone; a prior that is not rigid gets
 * ICPMI_ERR_INVALID_ARG and an identity.  status == NULL: the first error is the return value.  No scan is left staged (icpmi_map_update_staged
 * afterwards is ICPMI_ERR_INVALID_ARG) and there is no covariance, as after any batch. */
icpmi_status icpmi_register_multistart_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* priors, int32_t n_starts,
                                           int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status);
/* ... with the scan on the host: one upload (as icpmi_register_prior), then the call above */
icpmi_status icpmi_register_multistart(icpmi_handle h, const float* scan4, int64_t n, const float* priors, int32_t n_starts,
                                       int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status);
/* Test seam: the n-th value (n >= 1) of the std::minstd_rand stream as the DEVICE computes it by skip-ahead (csrc/ssn.hip, behind
 * SamplingSurfaceNormalDataPointsFilter -- PM::ICPSequence::setDefault(), Mapper.cpp:74-78).  [rand.predef]: seed 1, n = 10 000 -> 399268537. */
icpmi_status icpmi_debug_minstd_nth(icpmi_handle h, uint32_t seed, uint32_t n, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif
