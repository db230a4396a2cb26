"""Python-side mirror of ``PM::ICPSequence`` (the object behind ``Mapper::processInput``,
/root/reference norlab_icp_mapper/Mapper.h:23, Mapper.cpp:72,77,213,219; Map.cpp:111,178,528,581)
over the C ABI of libicpmi.so.  Same method names and error behaviour as the reference object so
that the parity tests read like tests of the reference would:

    icp = ICPSequence.loadFromYaml(chain)     # icp.loadFromYamlNode(node["icp"])
    icp.setMap(cloud, normals)                # bool, False on an empty cloud
    T = icp(scan)                             # 4x4 correction in the map frame
    icp.errorMinimizer.getOverlap()

Clouds are numpy float32 arrays of shape (N, 4) (== a 4 x N column-major ``features`` block),
normals (N, 3); transforms are ordinary 4x4 numpy matrices.  All compute happens in the HIP library.
"""
import ctypes as C
import math

import numpy as np

from . import _capi


class ConvergenceError(RuntimeError):
    """PM::ConvergenceError"""


class InvalidField(RuntimeError):
    """PM::DataPoints::InvalidField"""


class InvalidParameter(ValueError):
    """PM::Parametrizable::InvalidParameter"""


class TransformationError(ValueError):
    """PM::TransformationError"""


class HipError(RuntimeError):
    pass


_STATUS_EXC = {
    _capi.ERR_INVALID_ARG: InvalidParameter,
    _capi.ERR_HIP: HipError,
    _capi.ERR_NO_POINT_TO_MINIMIZE: ConvergenceError,
    _capi.ERR_NO_OUTLIER_TO_FILTER: ConvergenceError,
    _capi.ERR_BOUND: ConvergenceError,
    _capi.ERR_NAN: ConvergenceError,
    _capi.ERR_MISSING_NORMALS: InvalidField,
    _capi.ERR_UNSUPPORTED: NotImplementedError,
}

_OUTLIER_NAMES = {
    "MaxDistOutlierFilter": (_capi.OUT_MAXDIST, "maxDist", 1.0),
    "MinDistOutlierFilter": (_capi.OUT_MINDIST, "minDist", 1.0),
    "MedianDistOutlierFilter": (_capi.OUT_MEDIANDIST, "factor", 3.0),
    "TrimmedDistOutlierFilter": (_capi.OUT_TRIMMEDDIST, "ratio", 0.85),
    "SurfaceNormalOutlierFilter": (_capi.OUT_SURFACENORMAL, "maxAngle", 1.57),
}
_MINIMIZERS = {
    "IdentityErrorMinimizer": _capi.MIN_IDENTITY,
    "PointToPointErrorMinimizer": _capi.MIN_POINT_TO_POINT,
    "PointToPlaneErrorMinimizer": _capi.MIN_POINT_TO_PLANE,
    "PlaneToPlaneErrorMinimizer": _capi.MIN_PLANE_TO_PLANE,
    "SymmetricPointToPlaneErrorMinimizer": _capi.MIN_PLANE_TO_PLANE,  # (the same path under its other pair model: _PLANE_MODELS)
    "IntensityPointToPlaneErrorMinimizer": _capi.MIN_POINT_TO_PLANE,  # (point-to-plane with the photometric term: icpmi_set_intensity_weight)
}
INTENSITY_LAMBDA_DEFAULT, INTENSITY_KNN_DEFAULT, INTENSITY_DESC_DEFAULT = 0.968, 10, "intensity"
PLANE_EPSILON_DEFAULT = 1e-3
_PLANE_MODELS = {"gicp": _capi.PLANE_MODEL_GICP, "symmetric": _capi.PLANE_MODEL_SYMMETRIC}
_PLANE_MODEL_NAMES = {v: k for k, v in _PLANE_MODELS.items()}


def _check_plane_epsilon(eps):
    eps = float(eps)
    if not (math.isfinite(eps) and 0.0 < eps <= 1.0):
        raise InvalidParameter("PlaneToPlaneErrorMinimizer: epsilon must be finite and in (0, 1]")
    return eps



def _check_intensity_weight(w):
    w = float(w)
    if not (math.isfinite(w) and 0.0 <= w < 1.0):
        raise InvalidParameter("IntensityPointToPlaneErrorMinimizer: the intensity weight (1 - lambdaGeometric) must be finite and in [0, 1)")
    return w


def _check_intensity_knn(k):
    if int(k) != k or not 1 <= int(k) <= 31:
        raise InvalidParameter("IntensityPointToPlaneErrorMinimizer: gradientKnn must be an integer in [1, 31]")
    return int(k)


VOXEL_SIZE_DEFAULT = 1.0
# the C call's wording (csrc/api.hip: voxel_check), as the chain parser sees the same combinations
_VOXEL_REFUSAL = "register: the voxel matcher (icpmi_set_voxel_matcher > 0) "


def _check_voxel_size(size):
    size = float(size)
    if not (math.isfinite(size) and size >= 0.0):
        raise InvalidParameter("VoxelMatcher: voxelSize must be finite and >= 0 (0: off)")
    return size


VOXEL_MAX_LEVELS = 4


def _check_voxel_sizes(sizes):
    """The rules of icpmi_set_voxel_schedule: 1 to 4 sizes, each finite and > 0, strictly descending (coarsest first)."""
    if isinstance(sizes, (str, bytes)) or not hasattr(sizes, "__iter__"):
        raise InvalidParameter("VoxelMatcher: voxelSizes must be a list of 1 to 4 voxel sizes")
    try:
        sizes = [float(v) for v in sizes]
    except (TypeError, ValueError):
        raise InvalidParameter("VoxelMatcher: voxelSizes must be a list of numbers")
    if not 1 <= len(sizes) <= VOXEL_MAX_LEVELS:
        raise InvalidParameter("VoxelMatcher: voxelSizes takes 1 to 4 voxel sizes")
    if not all(math.isfinite(v) and v > 0.0 for v in sizes):
        raise InvalidParameter("VoxelMatcher: every voxel size of voxelSizes must be finite and > 0")
    if any(not b < a for a, b in zip(sizes, sizes[1:])):
        raise InvalidParameter("VoxelMatcher: voxelSizes must be strictly descending (coarsest first)")
    return sizes


def _check_plane_model(model):
    if model not in _PLANE_MODELS:
        raise InvalidParameter(f"plane_model must be one of {sorted(_PLANE_MODELS)}, not {model!r}")
    return model


def _f32c(a, cols):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != cols:
        raise InvalidParameter(f"expected an (N, {cols}) float32 array, got {a.shape}")
    return a


def _T_to_c(T):
    """4x4 numpy (row-major) -> column-major float[16]"""
    T = np.asarray(T, dtype=np.float32)
    return np.ascontiguousarray(T.T).ravel()


def _T_from_c(buf):
    return np.array(buf, dtype=np.float32).reshape(4, 4).T.copy()


def default_config(**kw):
    lib = _capi.load()
    cfg = _capi.Config()
    lib.icpmi_config_default(C.byref(cfg))
    outliers = kw.pop("outliers", None)
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise InvalidParameter(f"unknown config field {k}")
        setattr(cfg, k, v)
    if outliers is not None:
        cfg.n_outlier = len(outliers)
        for i, o in enumerate(outliers):  # (type, param[, iparam[, param2]])
            cfg.outlier[i].type = o[0]
            cfg.outlier[i].param = o[1]
            cfg.outlier[i].iparam = o[2] if len(o) > 2 else 0
            cfg.outlier[i].param2 = o[3] if len(o) > 3 else 0.0
            cfg.outlier[i].param3 = o[4] if len(o) > 4 else 0.0
    return cfg


def config_from_yaml_chain(chain, **engine):
    """Translate the ``icp:`` sub-tree of a mapper YAML (Mapper.cpp:72) into an icpmi_config.

    Only the modules on the hot path are accepted; anything else raises like libpointmatcher's
    registrar would for an unknown module.
    """
    chain = chain or {}
    kw = {}
    valid = {"matcher", "outlierFilters", "errorMinimizer", "transformationCheckers", "inspector", "logger",
             "readingDataPointsFilters", "referenceDataPointsFilters", "readingStepDataPointsFilters"}
    for key in chain:
        if key not in valid:
            raise InvalidParameter(f"unknown ICP chain key: {key}")
    for key in ("readingDataPointsFilters", "referenceDataPointsFilters", "readingStepDataPointsFilters"):
        if chain.get(key):
            raise NotImplementedError(f"{key} inside the ICP chain are not on the accelerated path; apply them as input filters")

    def single(node, what):
        if isinstance(node, str):
            return node, {}
        if isinstance(node, dict) and len(node) == 1:
            (name, params), = node.items()
            return name, (params or {})
        raise InvalidParameter(f"malformed {what} node: {node!r}")

    matcher = chain.get("matcher", {"KDTreeMatcher": {}})
    name, p = single(matcher, "matcher")
    max_dist_field = None
    voxel_size = None
    voxel_sizes = None
    if name == "VoxelMatcher":
        # voxelised plane-to-plane ICP (not libpointmatcher's; include/icpmi.h: icpmi_set_voxel_matcher): a reading point is paired with the
        # map voxel it falls into -- no search, hence no knn / maxDist / epsilon
        for key in p:
            if key not in ("voxelSize", "voxelSizes"):
                raise InvalidParameter(f"VoxelMatcher: unknown parameter {key}")
        if "voxelSize" in p and "voxelSizes" in p:
            raise InvalidParameter("VoxelMatcher: voxelSize and voxelSizes are one parameter said two ways: give one of them")
        if "voxelSizes" in p:  # a schedule, coarsest first (include/icpmi.h: icpmi_set_voxel_schedule)
            voxel_sizes = _check_voxel_sizes(p["voxelSizes"])
            voxel_size = voxel_sizes[-1]
        else:
            voxel_size = _check_voxel_size(p.get("voxelSize", VOXEL_SIZE_DEFAULT))
            if not voxel_size > 0.0:
                raise InvalidParameter("VoxelMatcher: voxelSize must be finite and > 0")
    elif name == "KDTreeVarDistMatcher":
        # every reading point searches within its own radius: the reading's 1-row descriptor `maxDistField` (ICPSequence.__call__ hands it over)
        for key in p:
            if key not in ("knn", "epsilon", "searchType", "maxDistField"):
                raise InvalidParameter(f"KDTreeVarDistMatcher: unknown parameter {key}")
        kw["knn"] = int(p.get("knn", 1))
        kw["epsilon"] = float(p.get("epsilon", 0))
        kw["var_dist"] = 1
        max_dist_field = str(p.get("maxDistField", "maxSearchDist"))
    elif name == "KDTreeMatcher":
        for key in p:
            if key not in ("knn", "epsilon", "searchType", "maxDist", "maxDistField"):
                raise InvalidParameter(f"KDTreeMatcher: unknown parameter {key}")
        kw["knn"] = int(p.get("knn", 1))
        kw["epsilon"] = float(p.get("epsilon", 0))
        md = p.get("maxDist", math.inf)
        kw["max_dist"] = math.inf if str(md) in ("inf", ".inf") else float(md)
    else:
        raise InvalidParameter(f"unknown matcher {name}")

    outs = []
    for node in chain.get("outlierFilters", []) or []:
        name, p = single(node, "outlier filter")
        if name == "GenericDescriptorOutlierFilter":
            # upstream defaults: source reference, descName none, useSoftThreshold 0, useLargerThan 1, threshold 0.1
            for key in p:
                if key not in ("source", "descName", "useSoftThreshold", "useLargerThan", "threshold"):
                    raise InvalidParameter(f"{name}: unknown parameter {key}")
            source = p.get("source", "reference")
            if source not in ("reference", "reading"):
                raise InvalidParameter(f"{name}: source must be reference or reading")
            # (source: reading -- r4: the reading's row goes to the device with ICPSequence.setReadingScalar before every registration)
            kw["generic_read_desc_name" if source == "reading" else "generic_desc_name"] = str(p.get("descName", "none"))
            flags = (_capi.GEN_SOFT if int(p.get("useSoftThreshold", 0)) else 0) | (_capi.GEN_LARGER if int(p.get("useLargerThan", 1)) else 0) | \
                    (_capi.GEN_SOURCE_READING if source == "reading" else 0)
            outs.append((_capi.OUT_GENERICDESCRIPTOR, float(p.get("threshold", 0.1)), flags, 0.0))
            continue
        if name == "VarTrimmedDistOutlierFilter":
            # upstream defaults: minRatio 0.05, maxRatio 0.99, lambda 0.95
            for key in p:
                if key not in ("minRatio", "maxRatio", "lambda"):
                    raise InvalidParameter(f"{name}: unknown parameter {key}")
            outs.append((_capi.OUT_VARTRIMMEDDIST, float(p.get("minRatio", 0.05)), 0, float(p.get("maxRatio", 0.99)), float(p.get("lambda", 0.95))))
            continue
        if name == "RobustOutlierFilter":
            # upstream defaults: robustFct cauchy, tuning 1, scaleEstimator mad, nbIterationForScale 0, distanceType point2point
            for key in p:
                if key not in ("robustFct", "tuning", "scaleEstimator", "nbIterationForScale", "distanceType", "approximation"):
                    raise InvalidParameter(f"{name}: unknown parameter {key}")
            fct, sc, dt = str(p.get("robustFct", "cauchy")), str(p.get("scaleEstimator", "mad")), str(p.get("distanceType", "point2point"))
            if fct not in _capi.ROBUST_FCT or dt not in _capi.ROBUST_DIST or sc not in ("none", "mad", "berg", "std"):
                raise InvalidParameter(f"{name}: unknown robustFct / scaleEstimator / distanceType")
            apx = float(str(p.get("approximation", "inf")).replace(".inf", "inf"))
            if not apx > 0.0:
                raise InvalidParameter(f"{name}: approximation must be > 0")
            outs.append((_capi.OUT_ROBUST, float(p.get("tuning", 1.0)),
                         _capi.ROBUST_FCT[fct] | (_capi.ROBUST_SCALE[sc] << 4) | (_capi.ROBUST_DIST[dt] << 8), float(int(p.get("nbIterationForScale", 0))), apx))
            continue
        if name not in _OUTLIER_NAMES:
            raise InvalidParameter(f"unknown outlier filter {name}")
        t, pname, default = _OUTLIER_NAMES[name]
        for key in p:
            if key != pname:
                raise InvalidParameter(f"{name}: unknown parameter {key}")
        outs.append((t, float(p.get(pname, default))))
    kw["outliers"] = outs
    if voxel_size is not None and outs:
        raise InvalidParameter(_VOXEL_REFUSAL + "is not served with outlier filters (a pair is a point and the voxel it falls into: there is no match distance to filter on)")

    name, p = single(chain.get("errorMinimizer", "PointToPlaneErrorMinimizer"), "errorMinimizer")
    if name == "PointToPlaneWithCovErrorMinimizer":
        # registers as PointToPlaneErrorMinimizer and leaves the pose covariance (errorMinimizer.getCovariance())
        for key in p:
            if key not in ("sensorStdDev", "force2D", "force4DOF", "degeneracyThreshold", "degeneracyAction"):
                raise InvalidParameter(f"{name}: unknown parameter {key}")
        kw["covariance"] = 1
        kw["sensor_std_dev"] = float(p.get("sensorStdDev", 0.01))
        name = "PointToPlaneErrorMinimizer"
    elif name == "PointToPlaneErrorMinimizer":
        for key in p:  # (a misspelt degeneracyThreshold must not leave the option off in silence)
            if key not in ("force2D", "force4DOF", "degeneracyThreshold", "degeneracyAction"):
                raise InvalidParameter(f"{name}: unknown parameter {key}")
    plane_epsilon = None
    if name == "PlaneToPlaneErrorMinimizer":
        # generalized ICP from the normals of both clouds (not libpointmatcher's; include/icpmi.h: ICPMI_MIN_PLANE_TO_PLANE)
        for key in p:
            if key not in ("epsilon", "force4DOF"):
                raise InvalidParameter(f"{name}: unknown parameter {key}")
        plane_epsilon = _check_plane_epsilon(p.get("epsilon", PLANE_EPSILON_DEFAULT))
    plane_model = None
    if name == "SymmetricPointToPlaneErrorMinimizer":
        # symmetric point-to-plane from the normals of both clouds (not libpointmatcher's; include/icpmi.h: ICPMI_PLANE_MODEL_SYMMETRIC)
        for key in p:
            if key != "force4DOF":
                raise InvalidParameter(f"{name}: unknown parameter {key}")
        plane_model = "symmetric"
    intensity = None
    if name == "IntensityPointToPlaneErrorMinimizer":
        # point-to-plane with a photometric term from one scalar descriptor of both clouds (not libpointmatcher's; include/icpmi.h:
        # icpmi_set_intensity_weight): lambdaGeometric in (0, 1], descName the descriptor, gradientKnn the neighbours of a map-side gradient
        for key in p:
            if key not in ("lambdaGeometric", "descName", "gradientKnn", "force4DOF"):
                raise InvalidParameter(f"{name}: unknown parameter {key}")
        lam = float(p.get("lambdaGeometric", INTENSITY_LAMBDA_DEFAULT))
        if not (math.isfinite(lam) and 0.0 < lam <= 1.0):
            raise InvalidParameter(f"{name}: lambdaGeometric must be finite and in (0, 1]")
        intensity = (_check_intensity_weight(1.0 - lam), _check_intensity_knn(p.get("gradientKnn", INTENSITY_KNN_DEFAULT)),
                     str(p.get("descName", INTENSITY_DESC_DEFAULT)))
    if name not in _MINIMIZERS:
        raise InvalidParameter(f"unknown error minimizer {name}")
    if voxel_size is not None and name == "SymmetricPointToPlaneErrorMinimizer":
        raise InvalidParameter(_VOXEL_REFUSAL + "is not served with the symmetric pair model (SymmetricPointToPlaneErrorMinimizer)")
    if voxel_size is not None and name != "PlaneToPlaneErrorMinimizer":
        raise InvalidParameter(_VOXEL_REFUSAL + "is defined on PlaneToPlaneErrorMinimizer only")
    if name == "PointToPlaneErrorMinimizer":
        # degeneracy-aware solve (not libpointmatcher's): degeneracyThreshold >= 0 (0 = off), degeneracyAction constrain | report
        thr = float(p.get("degeneracyThreshold", 0.0))
        action = str(p.get("degeneracyAction", "constrain"))
        if not (thr >= 0.0 and math.isfinite(thr)):
            raise InvalidParameter(f"{name}: degeneracyThreshold must be finite and >= 0")
        if action not in ("constrain", "report"):
            raise InvalidParameter(f"{name}: degeneracyAction must be constrain or report")
        if thr > 0.0 and int(p.get("force2D", 0)):
            raise InvalidParameter(f"{name}: degeneracyThreshold and force2D exclude each other")
        kw["degeneracy_threshold"] = thr if action == "constrain" else -thr
    kw["minimizer"] = _MINIMIZERS[name]
    kw["force_4dof"] = 1 if (name in ("PointToPlaneErrorMinimizer", "PlaneToPlaneErrorMinimizer", "SymmetricPointToPlaneErrorMinimizer", "IntensityPointToPlaneErrorMinimizer") and int(p.get("force4DOF", 0))) else 0
    kw["force_2d"] = 1 if (name == "PointToPlaneErrorMinimizer" and int(p.get("force2D", 0))) else 0
    if kw["force_4dof"] and kw["force_2d"]:
        raise InvalidParameter("PointToPlaneErrorMinimizer: force2D and force4DOF exclude each other")

    kw["max_iterations"] = 40
    for node in chain.get("transformationCheckers", [{"CounterTransformationChecker": {}}]) or []:
        name, p = single(node, "transformation checker")
        if name == "CounterTransformationChecker":
            kw["max_iterations"] = int(p.get("maxIterationCount", 40))
        elif name == "DifferentialTransformationChecker":
            kw["use_differential"] = 1
            kw["min_diff_rot"] = float(p.get("minDiffRotErr", 0.001))
            kw["min_diff_trans"] = float(p.get("minDiffTransErr", 0.001))
            kw["smooth_length"] = int(p.get("smoothLength", 3))
        elif name == "BoundTransformationChecker":
            kw["use_bound"] = 1
            kw["max_rot_norm"] = float(p.get("maxRotationNorm", 1))
            kw["max_trans_norm"] = float(p.get("maxTranslationNorm", 1))
        else:
            raise InvalidParameter(f"unknown transformation checker {name}")
    kw.update(engine)
    kw.pop("generic_desc_name", None)  # the caller hands the descriptor over with ICPSequence.setMapScalar
    kw.pop("generic_read_desc_name", None)  # ... and the reading's with ICPSequence.setReadingScalar
    cfg = default_config(**kw)
    if max_dist_field is not None:
        cfg.max_dist_field = max_dist_field  # (a Python attribute next to the C fields: the descriptor name is the host's business)
    if voxel_size is not None:
        cfg.voxel_size = voxel_size  # (likewise: ICPSequence hands it to icpmi_set_voxel_matcher)
    if voxel_sizes is not None:
        cfg.voxel_sizes = voxel_sizes  # (... and the schedule to icpmi_set_voxel_schedule)
    if plane_epsilon is not None:
        cfg.plane_epsilon = plane_epsilon  # (likewise: icpmi_config has no word left; ICPSequence hands it to icpmi_set_plane_epsilon)
    if plane_model is not None:
        cfg.plane_model = plane_model  # (likewise: ICPSequence hands it to icpmi_set_plane_pair_model)
    if intensity is not None:
        # (likewise: ICPSequence hands the weight to icpmi_set_intensity_weight; the descriptor's name and the knn are the host's business)
        cfg.intensity_weight, cfg.intensity_knn, cfg.intensity_desc_name = intensity
    return cfg


class Residual:
    """icpmi_residual as plain Python values (sum_abs = ErrorMinimizer::getResidualError())."""
    __slots__ = ("sum_abs", "sum_sq", "max_abs", "weighted_point_used_ratio", "weight_sum", "pairs", "trimmed_limit", "kind")

    def __init__(self, c):
        self.sum_abs, self.sum_sq, self.weight_sum = float(c.sum_abs), float(c.sum_sq), float(c.weight_sum)
        self.max_abs, self.weighted_point_used_ratio = np.float32(c.max_abs), np.float32(c.weighted_point_used_ratio)
        self.trimmed_limit = np.float32(c.trimmed_limit)
        self.pairs, self.kind = int(c.pairs), int(c.kind)

    def bits(self):
        """every field as raw bits (bit-for-bit comparisons)"""
        return (np.float64([self.sum_abs, self.sum_sq, self.weight_sum]).view(np.uint64).tolist(),
                np.float32([self.max_abs, self.weighted_point_used_ratio, self.trimmed_limit]).view(np.uint32).tolist(), self.pairs, self.kind)

    def __repr__(self):
        return "Residual(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


class SweepResult:
    """icpmi_sweep_result as plain Python values: T_begin / T_end (4, 4) float32, pose7 (2, 7) float64 (tx ty tz qx qy qz qw)."""
    __slots__ = ("T_begin", "T_end", "pose7", "iterations", "stop_reason", "pairs", "weight_sum", "sum_sq", "weighted_point_used_ratio",
                 "trimmed_limit")

    def __init__(self, c):
        self.T_begin, self.T_end = _T_from_c(c.T_begin[:]), _T_from_c(c.T_end[:])
        self.pose7 = np.array(c.pose7[:], dtype=np.float64).reshape(2, 7)
        self.iterations, self.stop_reason, self.pairs = int(c.iterations), int(c.stop_reason), int(c.pairs)
        self.weight_sum, self.sum_sq = float(c.weight_sum), float(c.sum_sq)
        self.weighted_point_used_ratio, self.trimmed_limit = np.float32(c.weighted_point_used_ratio), np.float32(c.trimmed_limit)

    def bits(self):
        """every field as raw bits (bit-for-bit comparisons)"""
        return (self.T_begin.view(np.uint32).tolist(), self.T_end.view(np.uint32).tolist(), self.pose7.view(np.uint64).tolist(), self.iterations,
                self.stop_reason, self.pairs, np.float64([self.weight_sum, self.sum_sq]).view(np.uint64).tolist(),
                np.float32([self.weighted_point_used_ratio, self.trimmed_limit]).view(np.uint32).tolist())

    def __repr__(self):
        return "SweepResult(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


def sweep_solve(sums, lambda_rot=0.0, lambda_trans=0.0, d=None):
    """icpmi_sweep_solve: host only, needs neither a handle nor a device.  sums (80,) as icpmi_sweep_sums lays them out, d (6,) the sum of
    xi_e - xi_b over earlier iterations (None: zero).  Returns x = (xi_b, xi_e) (12,) float64; ConvergenceError when the system is
    rank-deficient (a prior weight is needed) or holds no pair."""
    lib = _capi.load()
    s = np.ascontiguousarray(sums, dtype=np.float64).ravel()
    if s.shape[0] != 80:
        raise InvalidParameter(f"expected 80 sums, got {s.shape[0]}")
    dd = None if d is None else np.ascontiguousarray(d, dtype=np.float64).ravel()
    if dd is not None and dd.shape[0] != 6:
        raise InvalidParameter(f"expected d of 6 values, got {dd.shape[0]}")
    x = np.zeros(12, dtype=np.float64)
    P = C.POINTER(C.c_double)
    st = lib.icpmi_sweep_solve(s.ctypes.data_as(P), float(lambda_rot), float(lambda_trans), None if dd is None else dd.ctypes.data_as(P),
                               x.ctypes.data_as(P))
    if st != _capi.ICPMI_OK:
        raise _STATUS_EXC.get(st, RuntimeError)(lib.icpmi_last_error(None).decode())
    return x


class PoseScores:
    """What icpmi_residual_error_poses* returns: one Residual and one status per pose (a pose whose status is not 0 keeps an empty Residual),
    and `batched`, the number of poses that went through the batched launches."""

    def __init__(self, residuals, status, batched):
        self.residuals, self.status, self.batched = list(residuals), [int(s) for s in status], int(batched)

    def __len__(self):
        return len(self.residuals)

    def table(self):
        """(status, pairs, sum_abs) per pose: what rank_candidates reads"""
        return [(st, r.pairs, r.sum_abs) for st, r in zip(self.status, self.residuals)]

    def bits(self):
        return [(st, r.bits()) for st, r in zip(self.status, self.residuals)]


def rank_candidates(scores, n, min_pairs_ratio=0.5):
    """The order in which a relocalisation prefers its candidates.  scores: a PoseScores, or (status, pairs, sum_abs) per candidate; n: points
    of the reading.  A candidate whose status is not 0 or whose pairs < min_pairs_ratio * n (the ratio as float32, the product in
    double) is dropped; the rest come by sum_abs / pairs ascending (double), ties by the lower index.  Returns the list of indices."""
    table = scores.table() if isinstance(scores, PoseScores) else list(scores)
    need = float(np.float32(min_pairs_ratio)) * float(n)
    keyed = []
    for i, (st, pairs, sum_abs) in enumerate(table):
        if int(st) != 0 or int(pairs) <= 0 or float(int(pairs)) < need:
            continue
        keyed.append((float(sum_abs) / float(int(pairs)), i))
    keyed.sort()
    return [i for _, i in keyed]


class VoxelScore:
    """icpmi_voxel_score as plain Python values (likelihood = sum over the pairs of exp(-beta / 2 d^T M d))."""
    __slots__ = ("likelihood", "sum_maha", "pairs", "max_maha", "pairs_ratio", "level")

    def __init__(self, c):
        self.likelihood, self.sum_maha, self.pairs = float(c.likelihood), float(c.sum_maha), int(c.pairs)
        self.max_maha, self.pairs_ratio, self.level = np.float32(c.max_maha), np.float32(c.pairs_ratio), int(c.level)

    def bits(self):
        """every field as raw bits (bit-for-bit comparisons)"""
        return (np.float64([self.likelihood, self.sum_maha]).view(np.uint64).tolist(), self.pairs,
                np.float32([self.max_maha, self.pairs_ratio]).view(np.uint32).tolist(), self.level)

    def __repr__(self):
        return "VoxelScore(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


class VoxelPoseScores:
    """What icpmi_voxel_score_poses* returns: one VoxelScore and one status per pose (a pose that is not rigid keeps an empty score)."""

    def __init__(self, scores, status):
        self.scores, self.status = list(scores), [int(s) for s in status]

    def __len__(self):
        return len(self.scores)

    def table(self):
        """(status, pairs, likelihood) per pose: what rank_voxel_candidates reads"""
        return [(st, r.pairs, r.likelihood) for st, r in zip(self.status, self.scores)]

    def bits(self):
        return [(st, r.bits()) for st, r in zip(self.status, self.scores)]


def rank_voxel_candidates(scores, n, min_pairs_ratio=0.0):
    """The order in which a relocalisation on the voxel path prefers its candidates.  scores: a VoxelPoseScores, or (status, pairs,
    likelihood) per candidate; n: points of the reading.  A candidate whose status is not 0 or whose pairs < min_pairs_ratio * n (the ratio
    as float32, the product in double) is dropped; the rest come by likelihood / n descending (double), ties by the lower index.  Returns
    the list of indices."""
    table = scores.table() if isinstance(scores, VoxelPoseScores) else list(scores)
    need = float(np.float32(min_pairs_ratio)) * float(n)
    keyed = []
    for i, (st, pairs, lik) in enumerate(table):
        if int(st) != 0 or int(pairs) <= 0 or float(int(pairs)) < need:
            continue
        keyed.append((-(float(lik) / float(n)), i))
    keyed.sort()
    return [i for _, i in keyed]


def candidate_grid(pose, half_x, half_y, half_yaw, steps_x=1, steps_y=1, steps_yaw=1):
    """The start poses of a relocalisation around `pose` (4x4): translations pose.t + (dx, dy, 0) and rotations Rz(dyaw) pose.R with
    dx = half_x i / steps_x for i = -steps_x .. steps_x (likewise dy, dyaw; 0 steps: that axis stays), formed in double and rounded to
    float32.  `pose` itself comes first, then yaw outermost, y, x innermost, each ascending.  Returns (N, 4, 4) float32,
    N = (2 steps_x + 1)(2 steps_y + 1)(2 steps_yaw + 1)."""
    P = np.asarray(pose, dtype=np.float32).reshape(4, 4)
    if min(steps_x, steps_y, steps_yaw) < 0:
        raise InvalidParameter("candidate_grid: steps must be >= 0")
    out = [P.copy()]
    R = P[:3, :3].astype(np.float64)
    t = P[:3, 3].astype(np.float64)
    off = lambda half, k, steps: 0.0 if steps == 0 else float(half) * float(k) / float(steps)
    for ia in range(-steps_yaw, steps_yaw + 1):
        a = off(half_yaw, ia, steps_yaw)
        ca, sa = math.cos(a), math.sin(a)
        Rz = np.array([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]])
        for iy in range(-steps_y, steps_y + 1):
            for ix in range(-steps_x, steps_x + 1):
                if ia == 0 and iy == 0 and ix == 0:
                    continue
                C4 = P.copy()
                Rn = np.empty((3, 3))
                for r in range(3):
                    for c in range(3):
                        Rn[r, c] = (Rz[r, 0] * R[0, c] + Rz[r, 1] * R[1, c]) + Rz[r, 2] * R[2, c]
                C4[:3, :3] = Rn.astype(np.float32)
                C4[0, 3] = np.float32(t[0] + off(half_x, ix, steps_x))
                C4[1, 3] = np.float32(t[1] + off(half_y, iy, steps_y))
                out.append(C4)
    return np.stack(out).astype(np.float32)


def yaw_rotations(steps, roll=0.0, pitch=0.0):
    """The rotations of a search over the heading (globalLocalize): Rz(2 pi i / steps) Ry(pitch) Rx(roll) for i = 0 .. steps - 1, formed in
    double -- every entry of a product summed left to right -- and rounded to float32.  Returns (steps, 3, 3) float32."""
    if int(steps) < 1:
        raise InvalidParameter("yaw_rotations: steps must be >= 1")
    cr, sr, cp, sp = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
    Rx = [[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]]
    Ry = [[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]]
    mul = lambda A, B: [[(A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]
    Ryx = mul(Ry, Rx)
    out = np.empty((int(steps), 3, 3), dtype=np.float32)
    for i in range(int(steps)):
        a = 2.0 * math.pi * float(i) / float(int(steps))
        ca, sa = math.cos(a), math.sin(a)
        out[i] = np.array(mul([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]], Ryx), dtype=np.float64).astype(np.float32)
    return out


class GlobalLocalization:
    """What ICPSequence.globalLocalize returns (icpmi_global_localize_result): found, proven, rotation (index into the list), cell (a),
    score, points, pose (4x4 float32: [R_k | mu + s0 a]), levels, nodes_scored, leaves_scored, launches."""
    __slots__ = ("found", "proven", "rotation", "cell", "score", "points", "pose", "levels", "nodes_scored", "leaves_scored", "launches", "_raw")

    def __init__(self, c):
        self.found, self.proven, self.rotation, self.cell = bool(c.found), bool(c.proven), int(c.rotation), tuple(int(v) for v in c.cell)
        self.score, self.points, self.pose, self.levels = int(c.score), int(c.points), _T_from_c(c.T[:]), int(c.levels)
        self.nodes_scored, self.leaves_scored, self.launches = int(c.nodes_scored), int(c.leaves_scored), int(c.launches)
        self._raw = bytes(c)

    def bits(self):
        return self._raw

    def __repr__(self):
        return (f"GlobalLocalization(found={self.found}, proven={self.proven}, rotation={self.rotation}, cell={self.cell}, score={self.score}, "
                f"points={self.points}, levels={self.levels}, nodes_scored={self.nodes_scored}, launches={self.launches})")


def compose_pose(A, B):
    """A B for two 4x4 float32 matrices the way the host shell's Mat4 multiplies: every entry summed over k = 0 .. 3 in float32, one
    multiply and one add per term -- the same bits on both sides of the C ABI (host/Makefile compiles the shell with -ffp-contract=off
    for this: a fused multiply-add would round once where this rounds twice)."""
    A = np.asarray(A, dtype=np.float32).reshape(4, 4)
    B = np.asarray(B, dtype=np.float32).reshape(4, 4)
    S = np.zeros((4, 4), dtype=np.float32)
    for k in range(4):
        S = (S + (A[:, k:k + 1] * B[k:k + 1, :]).astype(np.float32)).astype(np.float32)
    return S


class Relocalization:
    """What ICPSequence.relocalize returns: the winner's corrected pose (4x4), its Residual, its index among the candidates and the
    PoseScores of all candidates.  `search`: the GlobalLocalization that supplied the candidate (relocalizeGlobal), else None."""
    __slots__ = ("pose", "residual", "index", "scores", "search")

    def __init__(self, pose, residual, index, scores):
        self.pose, self.residual, self.index, self.scores = pose, residual, int(index), scores
        self.search = None


class _ErrorMinimizerView:
    def __init__(self, owner):
        self._o = owner

    def getOverlap(self):
        """upstream: the sensor-noise count when the reading carried `simpleSensorNoise` and `normals` (ICPSequence.setReadingSensorNoise),
        the weighted ratio of used points otherwise"""
        sn = float(self._o.stats.sensor_noise_overlap)
        return sn if sn >= 0.0 else float(self._o.stats.weighted_point_used_ratio)

    def getPointUsedRatio(self):
        return float(self._o.stats.point_used_ratio)

    def getWeightedPointUsedRatio(self):
        return float(self._o.stats.weighted_point_used_ratio)

    def getCovariance(self):
        """PointToPlaneWithCovErrorMinimizer: the (6, 6) float32 covariance of the last single registration's pose, parameters
        (tx, ty, tz, alpha, beta, gamma), centred frame (include/icpmi.h: icpmi_get_covariance); NotImplementedError when there is none"""
        out = (C.c_float * 36)()
        self._o._check(self._o._lib.icpmi_get_covariance(self._o._h, out))
        return np.array(out[:], dtype=np.float32).reshape(6, 6).T.copy()

    def getLocalizability(self):
        """the degeneracy report of the last single registration (ICPSequence.localizability)"""
        return self._o.localizability()

    def getResidualError(self, reading, T=None):
        """ErrorMinimizer::getResidualError of `reading` against the map under the correction T (None: identity), by the chain's
        minimizer: the sum over the error elements of |p - q| (point-to-point) or |(p - q) . n| (point-to-plane) -- ICPSequence.residual"""
        return float(self._o.residual(reading, T).sum_abs)


class ICPSequence:
    """``PM::ICPSequence`` backed by one icpmi handle (one GPU, one stream)."""

    def __init__(self, cfg=None, plane_epsilon=None, plane_model=None, intensity_weight=None, intensity_knn=None, voxel_size=None, voxel_sizes=None, **kw):
        """plane_epsilon: epsilon of PlaneToPlaneErrorMinimizer (icpmi_set_plane_epsilon; default: the chain's, else 1e-3)
        plane_model: "gicp" | "symmetric", the pair model of minimizer 3 (icpmi_set_plane_pair_model; default: the chain's, else "gicp")
        intensity_weight: 1 - lambdaGeometric of the photometric term on minimizer 2 (icpmi_set_intensity_weight; default: the chain's, else 0 = off)
        intensity_knn: neighbours of a map-side intensity gradient, setMapIntensity's default (default: the chain's, else 10)
        voxel_size: VoxelMatcher's voxel size (icpmi_set_voxel_matcher; default: the chain's, else off)
        voxel_sizes: a schedule of 1 to 4 voxel sizes, coarsest first (icpmi_set_voxel_schedule; default: the chain's); not with voxel_size"""
        self._lib = _capi.load()
        self.cfg = cfg if cfg is not None else default_config(**kw)
        if plane_epsilon is None:
            plane_epsilon = getattr(self.cfg, "plane_epsilon", None)
        if plane_epsilon is not None:
            plane_epsilon = _check_plane_epsilon(plane_epsilon)
        if voxel_size is not None and voxel_sizes is not None:
            raise InvalidParameter("VoxelMatcher: voxel_size and voxel_sizes are one parameter said two ways: give one of them")
        if voxel_sizes is None and voxel_size is None:
            voxel_sizes = getattr(self.cfg, "voxel_sizes", None)
        if voxel_sizes is not None:
            voxel_sizes = _check_voxel_sizes(voxel_sizes)
        elif voxel_size is None:
            voxel_size = getattr(self.cfg, "voxel_size", None)
        if voxel_size is not None:
            voxel_size = _check_voxel_size(voxel_size)
        if plane_model is None:
            plane_model = getattr(self.cfg, "plane_model", None)
        if plane_model is not None:
            _check_plane_model(plane_model)
        if intensity_weight is None:
            intensity_weight = getattr(self.cfg, "intensity_weight", None)
        if intensity_weight is not None:
            intensity_weight = _check_intensity_weight(intensity_weight)
        if intensity_knn is None:
            intensity_knn = getattr(self.cfg, "intensity_knn", INTENSITY_KNN_DEFAULT)
        self.intensity_knn = _check_intensity_knn(intensity_knn)
        h = C.c_void_p()
        st = self._lib.icpmi_create(C.byref(self.cfg), C.byref(h))
        if st != _capi.ICPMI_OK:
            msg = self._lib.icpmi_last_error(None).decode()
            raise _STATUS_EXC.get(st, RuntimeError)(msg)
        self._h = h
        self.stats = _capi.Stats()
        self.errorMinimizer = _ErrorMinimizerView(self)
        self._last_n = 0
        self._intensity_on = False
        if plane_epsilon is not None:
            self.setPlaneEpsilon(plane_epsilon)
        if plane_model is not None:
            self.setPlaneModel(plane_model)
        if voxel_sizes is not None:
            self.setVoxelSchedule(voxel_sizes)
        elif voxel_size is not None:
            self.setVoxelMatcher(voxel_size)
        if intensity_weight is not None:
            self.setIntensityWeight(intensity_weight)

    @classmethod
    def loadFromYaml(cls, chain, **engine):
        return cls(config_from_yaml_chain(chain, **engine))

    def setConfig(self, cfg=None, **kw):
        """Swap the chain of the live handle (icpmi_set_config): the map and the handle stay valid."""
        new = cfg if cfg is not None else default_config(device=self.cfg.device, **kw)
        self._check(self._lib.icpmi_set_config(self._h, C.byref(new)))
        self.cfg = new

    def setPlaneEpsilon(self, eps):
        """icpmi_set_plane_epsilon: handle state (setConfig leaves it); the next registration runs with it"""
        self._check(self._lib.icpmi_set_plane_epsilon(self._h, float(eps)))

    def setVoxelMatcher(self, size):
        """icpmi_set_voxel_matcher: the voxel size of VoxelMatcher (0: off); handle state (setConfig leaves it).  Served with minimizer 3
        and plane_model "gicp", no outlier filter, by __call__ / registerFixed / minimizeStep with read_normals"""
        self._check(self._lib.icpmi_set_voxel_matcher(self._h, _check_voxel_size(size)))

    def getVoxelMatcher(self):
        out = C.c_float(0)
        self._check(self._lib.icpmi_get_voxel_matcher(self._h, C.byref(out)))
        return out.value

    def setVoxelSchedule(self, sizes):
        """icpmi_set_voxel_schedule: 1 to 4 voxel sizes, strictly descending -- the registration runs them coarse to fine, every level on the
        chain's checkers, the level switch on the device; an empty list switches the matcher off.  Handle state like
        setVoxelMatcher, which is a schedule of one."""
        sizes = _check_voxel_sizes(sizes) if len(sizes) else []
        arr = (C.c_float * max(1, len(sizes)))(*sizes)
        self._check(self._lib.icpmi_set_voxel_schedule(self._h, arr, len(sizes)))

    def getVoxelSchedule(self):
        arr, n = (C.c_float * VOXEL_MAX_LEVELS)(), C.c_int32(0)
        self._check(self._lib.icpmi_get_voxel_schedule(self._h, arr, C.byref(n)))
        return [arr[i] for i in range(n.value)]

    def voxelScheduleReport(self):
        """icpmi_get_voxel_schedule_report of the last registration: a list with one (iterations, pairs_first, pairs_last) per level entered"""
        lv = C.c_int32(0)
        it, pf, pl = ((C.c_int32 * VOXEL_MAX_LEVELS)() for _ in range(3))
        self._check(self._lib.icpmi_get_voxel_schedule_report(self._h, C.byref(lv), it, pf, pl))
        return [(it[i], pf[i], pl[i]) for i in range(lv.value)]

    def voxelMap(self, level=None):
        """icpmi_get_voxel_map: (ijk (V, 3) int32, mean (V, 3) in the centred frame, moments (V, 6): xx xy xz yy yz zz, count (V,)) in
        ascending key order; level: of the schedule (0 = the coarsest; icpmi_get_voxel_map_level), None = the finest"""
        def call(cap, *arrs):
            if level is None:
                return self._lib.icpmi_get_voxel_map(self._h, cap, *arrs, C.byref(nv))
            return self._lib.icpmi_get_voxel_map_level(self._h, int(level), cap, *arrs, C.byref(nv))
        nv = C.c_int64(0)
        st = call(0, None, None, None, None)
        if nv.value == 0:
            self._check(st)
        v = nv.value
        ijk, mean = np.zeros((v, 3), np.int32), np.zeros((v, 3), np.float32)
        mom, cnt = np.zeros((v, 6), np.float32), np.zeros(v, np.int32)
        self._check(call(v, ijk.ctypes.data, mean.ctypes.data, mom.ctypes.data, cnt.ctypes.data))
        return ijk, mean, mom, cnt

    def voxelLookup(self, q_centred, level=None):
        """icpmi_voxel_lookup: for (N, 3) or (N, 4) centred-frame points the index into voxelMap()'s order, -1 for no voxel; level as for
        voxelMap (icpmi_voxel_lookup_level)"""
        q = np.asarray(q_centred, np.float32)
        q4 = np.ones((q.shape[0], 4), np.float32)
        q4[:, :q.shape[1]] = q
        out = np.full(q.shape[0], -2, np.int32)
        if level is None:
            self._check(self._lib.icpmi_voxel_lookup(self._h, q4.ctypes.data, q4.shape[0], out.ctypes.data))
        else:
            self._check(self._lib.icpmi_voxel_lookup_level(self._h, int(level), q4.ctypes.data, q4.shape[0], out.ctypes.data))
        return out

    def setPlaneModel(self, model):
        """icpmi_set_plane_pair_model ("gicp" | "symmetric"): handle state (setConfig leaves it); the next registration runs with it"""
        self._check(self._lib.icpmi_set_plane_pair_model(self._h, _PLANE_MODELS[_check_plane_model(model)]))

    def getPlaneModel(self):
        out = C.c_int32(0)
        self._check(self._lib.icpmi_get_plane_pair_model(self._h, C.byref(out)))
        return _PLANE_MODEL_NAMES[int(out.value)]

    def getPlaneEpsilon(self):
        out = C.c_float(0)
        self._check(self._lib.icpmi_get_plane_epsilon(self._h, C.byref(out)))
        return float(out.value)

    # ---- the photometric term on point-to-plane (IntensityPointToPlaneErrorMinimizer; include/icpmi.h: icpmi_set_intensity_weight) ----
    def setIntensityWeight(self, w):
        """icpmi_set_intensity_weight (1 - lambdaGeometric, 0 = off): handle state (setConfig leaves it); the next registration runs with it"""
        self._check(self._lib.icpmi_set_intensity_weight(self._h, float(w)))
        self._intensity_on = float(w) > 0.0

    def getIntensityWeight(self):
        out = C.c_float(0)
        self._check(self._lib.icpmi_get_intensity_weight(self._h, C.byref(out)))
        return float(out.value)

    def setMapIntensity(self, intensity, knn=None):
        """icpmi_set_map_intensity: one intensity per point of the resident map, in the order setMap took them; the gradients (knn nearest other
        points each, default intensity_knn) are computed on the device.  Every change of the map drops the channel."""
        row = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1)
        st = self._lib.icpmi_set_map_intensity(self._h, row.ctypes.data, row.shape[0], _check_intensity_knn(self.intensity_knn if knn is None else knn))
        self._check(st)

    def setReadingIntensity(self, intensity):
        """icpmi_set_reading_intensity: the intensity row of the NEXT reading (one shot, like setReadingScalar)"""
        row = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1)
        self._check(self._lib.icpmi_set_reading_intensity(self._h, row.ctypes.data, row.shape[0]))

    def intensityGradient(self, cloud, normals, intensity, knn=None):
        """icpmi_intensity_gradient: the (N, 3) tangent-plane intensity gradients of a cloud with normals, as setMapIntensity computes them"""
        cloud, normals = _f32c(cloud, 4), _f32c(normals, 3)
        row = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1)
        if normals.shape[0] != cloud.shape[0] or row.shape[0] != cloud.shape[0]:
            raise InvalidParameter("normals / intensity / cloud size mismatch")
        out = np.zeros((cloud.shape[0], 3), dtype=np.float32)
        self._check(self._lib.icpmi_intensity_gradient(self._h, cloud.ctypes.data, cloud.shape[0], normals.ctypes.data, row.ctypes.data,
                                                       _check_intensity_knn(self.intensity_knn if knn is None else knn), out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.icpmi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != _capi.ICPMI_OK:
            msg = self._lib.icpmi_last_error(self._h).decode()
            raise _STATUS_EXC.get(st, RuntimeError)(msg)

    # ---- PM::ICPSequence surface ----
    def setMap(self, cloud, normals=None):
        cloud = _f32c(cloud, 4)
        acc = C.c_int32(0)
        nptr = None
        if normals is not None:
            normals = _f32c(normals, 3)
            if normals.shape[0] != cloud.shape[0]:
                raise InvalidParameter("normals / cloud size mismatch")
            nptr = normals.ctypes.data
        self._check(self._lib.icpmi_set_map(self._h, cloud.ctypes.data, cloud.shape[0], nptr, C.byref(acc)))
        return bool(acc.value)

    def setMapDev(self, d_cloud_ptr, m, d_normals_ptr=None):
        acc = C.c_int32(0)
        self._check(self._lib.icpmi_set_map_dev(self._h, d_cloud_ptr, m, d_normals_ptr, C.byref(acc)))
        return bool(acc.value)

    def hasMap(self):
        return bool(self._lib.icpmi_has_map(self._h))

    def getMapMean(self):
        out = (C.c_float * 3)()
        self._check(self._lib.icpmi_get_map_mean(self._h, out))
        return np.array(out[:], dtype=np.float32)

    def __call__(self, scan, scan_normals=None, descriptors=None):
        """descriptors: {name: rows} of the reading (rows: (N,) or (rows, N)).  A KDTreeVarDistMatcher chain takes its `maxDistField` row from
        there (InvalidField when it is missing or has more than one row), unless setReadingMaxDist armed one already; with an intensity
        weight set, the chain's intensity descriptor (default `intensity`) is armed from there as setReadingIntensity does."""
        scan = _f32c(scan, 4)
        nptr = None
        if scan_normals is not None:
            scan_normals = _f32c(scan_normals, 3)
            nptr = scan_normals.ctypes.data
        if self.cfg.var_dist and descriptors is not None:
            field = getattr(self.cfg, "max_dist_field", "maxSearchDist")
            if field not in descriptors:
                raise InvalidField(f"KDTreeVarDistMatcher: the reading has no descriptor {field}")
            row = np.asarray(descriptors[field], dtype=np.float32)
            if row.ndim == 2 and row.shape[0] == 1:
                row = row[0]
            if row.ndim != 1:
                raise InvalidField(f"KDTreeVarDistMatcher: descriptor {field} must have one row, got shape {row.shape}")
            self.setReadingMaxDist(row)
        if self._intensity_on and descriptors is not None:  # IntensityPointToPlaneErrorMinimizer: the chain's descName row, unless setReadingIntensity armed one
            field = getattr(self.cfg, "intensity_desc_name", INTENSITY_DESC_DEFAULT)
            if field in descriptors:
                self.setReadingIntensity(descriptors[field])
        T = (C.c_float * 16)()
        self._last_n = scan.shape[0]
        st = self._lib.icpmi_register(self._h, scan.ctypes.data, scan.shape[0], nptr, T, C.byref(self.stats))
        if st == _capi.ERR_INVALID_ARG and (self.cfg.var_dist or self._intensity_on):  # (a missing descriptor row is upstream's InvalidField)
            msg = self._lib.icpmi_last_error(self._h).decode()
            if msg.startswith("InvalidField"):
                raise InvalidField(msg)
        self._check(st)
        return _T_from_c(T[:])

    # ---- which directions the last registration constrained (icpmi_get_localizability; errorMinimizer.getCovariance() is its neighbour) ----
    def localizability(self):
        """icpmi_get_localizability as a dict (degeneracy_threshold != 0): n, n_degenerate, degenerate (n bools), eigval (n, mu ascending),
        basis ((6, n) float64, column e = eigenvector e in the pivoted, scaled coordinates), pivot (3, map frame), lnorm, weight_sum, pairs,
        iterations -- of the last counted iteration of the last single registration; NotImplementedError when there is none"""
        r = _capi.Localizability()
        self._check(self._lib.icpmi_get_localizability(self._h, C.byref(r)))
        n = int(r.n)
        return dict(n=n, n_degenerate=int(r.n_degenerate), degenerate=np.array(r.degenerate[:n], dtype=bool),
                    eigval=np.array(r.eigval[:n], dtype=np.float64), basis=np.array(r.basis[:], dtype=np.float64).reshape(6, 6).T[:, :n].copy(),
                    pivot=np.array(r.pivot[:], dtype=np.float64), lnorm=float(r.lnorm), weight_sum=float(r.weight_sum), pairs=int(r.pairs),
                    iterations=int(r.iterations))

    # ---- how well a reading fits the map under a given pose (icpmi_residual_error*) ----
    def _residual_out(self, st, res):
        if st == _capi.ERR_INVALID_ARG:
            msg = self._lib.icpmi_last_error(self._h).decode()
            if msg.startswith("InvalidField"):
                raise InvalidField(msg)
            if msg.startswith("TransformationError"):
                raise TransformationError(msg)
        self._check(st)
        return Residual(res)

    def residual(self, reading, T=None, normals=None, kind=0):
        """icpmi_residual_error: `reading` (N, 4), already moved by the prior as for __call__, matched once against the map under the
        correction T (4x4, None: identity) and weighed by the chain's outlier filters.  kind 0: by the chain's minimizer, 1: point-to-point,
        2: point-to-plane.  normals (N, 3): the reading's, for a SurfaceNormalOutlierFilter.  Returns a Residual: sum_abs
        (getResidualError()), sum_sq, max_abs, pairs, weight_sum, weighted_point_used_ratio, trimmed_limit, kind."""
        scan = _f32c(reading, 4)
        nptr = None
        if normals is not None:
            normals = _f32c(normals, 3)
            nptr = normals.ctypes.data
        Tc = None if T is None else _T_to_c(T)
        res = _capi.Residual()
        st = self._lib.icpmi_residual_error(self._h, scan.ctypes.data, scan.shape[0], nptr, None if Tc is None else Tc.ctypes.data, int(kind),
                                            C.byref(res))
        return self._residual_out(st, res)

    def residualDev(self, d_scan_ptr, n, T=None, d_normals_ptr=None, kind=0):
        """icpmi_residual_error_dev: residual() for a reading (and its normals) already in HBM."""
        Tc = None if T is None else _T_to_c(T)
        res = _capi.Residual()
        st = self._lib.icpmi_residual_error_dev(self._h, d_scan_ptr, int(n), d_normals_ptr, None if Tc is None else Tc.ctypes.data, int(kind),
                                                C.byref(res))
        return self._residual_out(st, res)

    def residualStaged(self, T=None, kind=0):
        """icpmi_residual_error_staged: residual() of the scan registerWithPrior left in HBM (no upload), under the correction T."""
        Tc = None if T is None else _T_to_c(T)
        res = _capi.Residual()
        st = self._lib.icpmi_residual_error_staged(self._h, None if Tc is None else Tc.ctypes.data, int(kind), C.byref(res))
        return self._residual_out(st, res)

    # ---- the same reading under many poses, and relocalisation from them (icpmi_residual_error_poses*, icpmi_register_multistart*) ----
    @staticmethod
    def _poses_to_c(poses):
        P = np.asarray(poses, dtype=np.float32)
        if P.ndim == 2:
            P = P[None]
        if P.ndim != 3 or P.shape[1:] != (4, 4):
            raise InvalidParameter(f"expected (P, 4, 4) poses, got {P.shape}")
        return np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(-1)  # column-major, 16 floats per pose

    def _poses_out(self, st, res, status, batched):
        if st == _capi.ERR_INVALID_ARG:
            msg = self._lib.icpmi_last_error(self._h).decode()
            if msg.startswith("InvalidField"):
                raise InvalidField(msg)
        self._check(st)
        return PoseScores([Residual(r) for r in res], [int(x) for x in status], batched.value)

    def residuals(self, reading, poses, normals=None, kind=0):
        """icpmi_residual_error_poses: residual(reading, T) for every T of `poses` (P, 4, 4) in one call -- the reading uploaded, centred and
        sorted once, the poses in chunks of 16 through batched launches where the chain allows.  Returns a PoseScores; errors of one pose
        (a matrix that is not rigid, nothing to filter, no pair) are in its status, errors of the whole call raise."""
        scan = _f32c(reading, 4)
        nptr = None
        if normals is not None:
            normals = _f32c(normals, 3)
            nptr = normals.ctypes.data
        Tc = self._poses_to_c(poses)
        P = Tc.shape[0] // 16
        res = (_capi.Residual * max(P, 1))()
        status = (C.c_int * max(P, 1))()
        batched = C.c_int32(0)
        st = self._lib.icpmi_residual_error_poses(self._h, scan.ctypes.data, scan.shape[0], nptr, Tc.ctypes.data, P, int(kind), res, status,
                                                  C.byref(batched))
        return self._poses_out(st, res[:P], status[:P], batched)

    def residualsDev(self, d_scan_ptr, n, poses, d_normals_ptr=None, kind=0):
        """icpmi_residual_error_poses_dev: residuals() for a reading (and its normals) already in HBM."""
        Tc = self._poses_to_c(poses)
        P = Tc.shape[0] // 16
        res = (_capi.Residual * max(P, 1))()
        status = (C.c_int * max(P, 1))()
        batched = C.c_int32(0)
        st = self._lib.icpmi_residual_error_poses_dev(self._h, d_scan_ptr, int(n), d_normals_ptr, Tc.ctypes.data, P, int(kind), res, status,
                                                      C.byref(batched))
        return self._poses_out(st, res[:P], status[:P], batched)

    def _require_bare_reading_chain(self, who):
        """icpmi_register_multistart carries the points alone, as icpmi_register_prior does: a chain that reads the reading's normals or one
        of its descriptor rows cannot go through it (residuals serves such chains)"""
        for f in range(self.cfg.n_outlier):
            o = self.cfg.outlier[f]
            if o.type == 5:
                raise InvalidParameter(f"{who}: the chain's SurfaceNormalOutlierFilter reads the reading's normals, which the multistart registration does not carry")
            if o.type == 6 and (o.iparam & 1):
                raise InvalidParameter(f"{who}: the chain's GenericDescriptorOutlierFilter reads a descriptor row of the reading, which the multistart registration does not carry")
        if self.cfg.var_dist:
            raise InvalidParameter(f"{who}: KDTreeVarDistMatcher reads the reading's maxDistField row, which the multistart registration does not carry")

    def _multistart(self, fn, scan_ptr, n, priors, fixed_iterations):
        self._require_bare_reading_chain("registerMultiStart")
        Tc = self._poses_to_c(priors)
        S = Tc.shape[0] // 16
        T = (C.c_float * (16 * max(S, 1)))()
        stats = (_capi.Stats * max(S, 1))()
        status = (C.c_int * max(S, 1))()
        self._check(fn(self._h, scan_ptr, int(n), Tc.ctypes.data, S, int(fixed_iterations), T, stats, status))
        return [_T_from_c(T[16 * s:16 * s + 16]) for s in range(S)], [stats[s] for s in range(S)], [int(status[s]) for s in range(S)]

    def registerMultiStartDev(self, d_scan_ptr, n, priors, fixed_iterations=0):
        """icpmi_register_multistart_dev: the sensor-frame scan in HBM registered from every prior of `priors` (S <= 16, (S, 4, 4)) at once.
        Returns (list of 4x4 corrections, list of Stats, list of status codes), each start as registerWithPrior alone."""
        return self._multistart(self._lib.icpmi_register_multistart_dev, d_scan_ptr, n, priors, fixed_iterations)

    def registerMultiStart(self, scan, priors, fixed_iterations=0):
        """icpmi_register_multistart: registerMultiStartDev for a scan on the host (one upload)."""
        scan = _f32c(scan, 4)
        return self._multistart(self._lib.icpmi_register_multistart, scan.ctypes.data, scan.shape[0], priors, fixed_iterations)

    def relocalize(self, reading, candidates, min_pairs_ratio=0.5, refine=4, kind=0):
        """Where is the sensor, given candidate poses?  Every candidate is scored (residuals), the failed ones and those with fewer than
        min_pairs_ratio * N pairs are dropped, the rest ranked by sum_abs / pairs (rank_candidates); the best `refine` (<= 16) are refined
        (registerMultiStart), the refined poses scored once more and ranked by the same rule.  Returns a Relocalization; ConvergenceError
        when no candidate survives."""
        scan = _f32c(reading, 4)
        cand = np.asarray(candidates, dtype=np.float32).reshape(-1, 4, 4)
        if cand.shape[0] == 0:
            raise InvalidParameter("relocalize: no candidates")
        self._require_bare_reading_chain("relocalize")  # (before anything is scored: the refinement could not run)
        n = scan.shape[0]
        scores = self.residuals(scan, cand, kind=kind)
        order = rank_candidates(scores, n, min_pairs_ratio)
        if not order:
            raise ConvergenceError("relocalize: no candidate survived the scoring")
        best = order[:max(1, min(int(refine), 16))]
        corr, _, status = self.registerMultiStart(scan, cand[best])
        refined = np.stack([compose_pose(corr[i], cand[best[i]]) for i in range(len(best))])
        again = self.residuals(scan, refined, kind=kind)
        again.status = [a if s == 0 else s for a, s in zip(again.status, status)]  # a start that did not converge is out
        final = rank_candidates(again, n, min_pairs_ratio)
        if not final:
            raise ConvergenceError("relocalize: no refined candidate survived the scoring")
        w = final[0]
        return Relocalization(refined[w].copy(), again.residuals[w], best[w], scores)

    # ---- the same on the voxel path: poses scored by table lookup (icpmi_voxel_score_poses*) ----
    def _voxel_scores(self, fn, scan_ptr, n, nptr, poses, level, beta):
        Tc = self._poses_to_c(poses)
        P = Tc.shape[0] // 16
        opts = _capi.VoxelScoreOptions()
        self._lib.icpmi_voxel_score_options_default(C.byref(opts))
        opts.level, opts.beta = (-1 if level is None else int(level)), float(beta)
        res = (_capi.VoxelScore * max(P, 1))()
        status = (C.c_int * max(P, 1))()
        self._check(fn(self._h, scan_ptr, int(n), nptr, Tc.ctypes.data, P, C.byref(opts), res, status))
        return VoxelPoseScores([VoxelScore(r) for r in res[:P]], status[:P])

    def voxelScores(self, reading, normals, poses, level=None, beta=1.0):
        """icpmi_voxel_score_poses: for every T of `poses` (P, 4, 4; P <= 4096) the bounded likelihood of `reading` (N, 4) with `normals`
        (N, 3) against the voxel table of `level` (None: the finest; 0: the coarsest of a schedule) -- one upload, one scoring launch, no
        matcher.  Returns a VoxelPoseScores; errors of one pose (not rigid, no pair) are in its status, errors of the whole call raise."""
        scan = _f32c(reading, 4)
        nptr = None
        if normals is not None:
            normals = _f32c(normals, 3)
            if normals.shape[0] != scan.shape[0]:
                raise InvalidParameter("normals / cloud size mismatch")
            nptr = normals.ctypes.data
        return self._voxel_scores(self._lib.icpmi_voxel_score_poses, scan.ctypes.data, scan.shape[0], nptr, poses, level, beta)

    def voxelScoresDev(self, d_scan_ptr, n, d_normals_ptr, poses, level=None, beta=1.0):
        """icpmi_voxel_score_poses_dev: voxelScores() for a reading and its normals already in HBM."""
        return self._voxel_scores(self._lib.icpmi_voxel_score_poses_dev, d_scan_ptr, n, d_normals_ptr, poses, level, beta)

    # ---- many readings, or many starts, in one loop on the voxel path (icpmi_voxel_register_*) ----
    def voxelRegisterBatchDev(self, d_scan_ptrs, ns, d_normals_ptrs, fixed_iterations=0):
        """icpmi_voxel_register_batch_dev: B <= 16 readings in HBM (device pointers, sizes) with their normals (device pointers, 3 floats
        per point) against the map of a VoxelMatcher handle in one loop; every reading to the bits registerDev gives it alone.
        Returns (list of 4x4 corrections, list of Stats, list of status codes)."""
        B = len(d_scan_ptrs)
        if len(ns) != B or len(d_normals_ptrs) != B:
            raise InvalidParameter("voxelRegisterBatchDev: one size and one normals pointer per reading")
        ptrs = (C.c_void_p * max(B, 1))(*[None if p is None else int(p) for p in d_scan_ptrs])
        nptrs = (C.c_void_p * max(B, 1))(*[None if p is None else int(p) for p in d_normals_ptrs])
        nn = (C.c_int64 * max(B, 1))(*[int(n) for n in ns])
        T = (C.c_float * (16 * max(B, 1)))()
        stats = (_capi.Stats * max(B, 1))()
        status = (C.c_int * max(B, 1))()
        self._check(self._lib.icpmi_voxel_register_batch_dev(self._h, B, ptrs, nn, nptrs, int(fixed_iterations), T, stats, status))
        self.batch_stats = stats
        return [_T_from_c(T[16 * b:16 * b + 16]) for b in range(B)], [stats[b] for b in range(B)], [int(status[b]) for b in range(B)]

    def _voxel_multistart(self, fn, scan_ptr, n, nptr, priors, fixed_iterations):
        Tc = self._poses_to_c(priors)
        S = Tc.shape[0] // 16
        T = (C.c_float * (16 * max(S, 1)))()
        stats = (_capi.Stats * max(S, 1))()
        status = (C.c_int * max(S, 1))()
        self._check(fn(self._h, scan_ptr, int(n), nptr, Tc.ctypes.data, S, int(fixed_iterations), T, stats, status))
        return [_T_from_c(T[16 * s:16 * s + 16]) for s in range(S)], [stats[s] for s in range(S)], [int(status[s]) for s in range(S)]

    def voxelRegisterMultiStartDev(self, d_scan_ptr, n, d_normals_ptr, priors, fixed_iterations=0):
        """icpmi_voxel_register_multistart_dev: the reading and its normals in HBM registered from every prior of `priors` (S <= 16,
        (S, 4, 4)) in one loop; start s is transform(priors[s]) followed by the registration of the result, bit for bit.
        Returns (list of 4x4 corrections, list of Stats, list of status codes); composing with the prior stays the caller's."""
        return self._voxel_multistart(self._lib.icpmi_voxel_register_multistart_dev, d_scan_ptr, n, d_normals_ptr, priors, fixed_iterations)

    def voxelRegisterMultiStart(self, reading, normals, priors, fixed_iterations=0):
        """icpmi_voxel_register_multistart: voxelRegisterMultiStartDev for a reading on the host (one upload of it and its normals)."""
        scan = _f32c(reading, 4)
        nptr = None
        if normals is not None:
            normals = _f32c(normals, 3)
            if normals.shape[0] != scan.shape[0]:
                raise InvalidParameter("normals / cloud size mismatch")
            nptr = normals.ctypes.data
        return self._voxel_multistart(self._lib.icpmi_voxel_register_multistart, scan.ctypes.data, scan.shape[0], nptr, priors, fixed_iterations)

    def voxel_batch_report(self, member):
        """icpmi_get_voxel_batch_report: what voxelScheduleReport() answers, for member `member` (start `member`) of the last voxel batch
        or multistart: a list with one (iterations, pairs_first, pairs_last) per level entered"""
        lv = C.c_int32(0)
        it, pf, pl = ((C.c_int32 * VOXEL_MAX_LEVELS)() for _ in range(3))
        self._check(self._lib.icpmi_get_voxel_batch_report(self._h, int(member), C.byref(lv), it, pf, pl))
        return [(it[i], pf[i], pl[i]) for i in range(lv.value)]

    def relocalizeVoxel(self, reading, normals, candidates, refine=4, level=0, beta=1.0, min_pairs_ratio=0.0):
        """Where is the sensor, given candidate poses -- on a VoxelMatcher handle.  Every candidate is scored at `level` (0: the coarsest
        level of a schedule, the widest basin) and ranked (rank_voxel_candidates); the reading moved by each of the best `refine` is
        registered by the handle's own chain, the whole schedule, all starts in one loop (voxelRegisterMultiStart, chunks of 16); the
        refined poses are scored at the finest level and ranked again.  Returns a Relocalization whose `residual` is the winner's
        VoxelScore; ConvergenceError when nothing survives."""
        scan, nrm = _f32c(reading, 4), _f32c(normals, 3)
        cand = np.asarray(candidates, dtype=np.float32).reshape(-1, 4, 4)
        if cand.shape[0] == 0:
            raise InvalidParameter("relocalizeVoxel: no candidates")
        n = scan.shape[0]
        scores = self.voxelScores(scan, nrm, cand, level=level, beta=beta)
        order = rank_voxel_candidates(scores, n, min_pairs_ratio)
        if not order:
            raise ConvergenceError("relocalizeVoxel: no candidate survived the scoring")
        best = order[:max(1, int(refine))]
        refined, status = [], []
        soft = (_capi.ERR_NO_POINT_TO_MINIMIZE, _capi.ERR_NO_OUTLIER_TO_FILTER, _capi.ERR_BOUND, _capi.ERR_NAN)
        for c0 in range(0, len(best), 16):  # one multistart call per chunk of 16: every start is bit for bit transform + icpmi_register
            chunk = best[c0:c0 + 16]
            corr, sts, status_c = self.voxelRegisterMultiStart(scan, nrm, cand[chunk])
            self._last_n = n
            C.memmove(C.byref(self.stats), C.byref(sts[-1]), C.sizeof(_capi.Stats))  # (the last refined start's, as start after start left it)
            for j, i in enumerate(chunk):
                st = status_c[j]
                if st in soft:
                    refined.append(cand[i].copy())  # a start that did not converge is out, under the status it ended with
                    status.append(int(st))
                    continue
                if st != _capi.ICPMI_OK:
                    raise _STATUS_EXC.get(st, RuntimeError)(f"relocalizeVoxel: the refinement of candidate {i} ended with status {st}")
                refined.append(compose_pose(corr[j], cand[i]))
                status.append(0)
        refined = np.stack(refined)
        again = self.voxelScores(scan, nrm, refined, level=None, beta=beta)
        again.status = [a if s == 0 else s for a, s in zip(again.status, status)]  # a start that did not converge is out
        final = rank_voxel_candidates(again, n, min_pairs_ratio)
        if not final:
            raise ConvergenceError("relocalizeVoxel: no refined candidate survived the scoring")
        w = final[0]
        return Relocalization(refined[w].copy(), again.scores[w], best[w], scores)

    # ---- a search without candidates: branch and bound over occupancy levels (icpmi_global_localize*) ----
    @staticmethod
    def _rotations_to_c(rotations):
        """(K, 3, 3) rotation matrices -> K column-major blocks of 9 floats"""
        R = np.asarray(rotations, dtype=np.float32).reshape(-1, 3, 3)
        return np.ascontiguousarray(np.transpose(R, (0, 2, 1))).reshape(-1)

    def _global_localize_options(self, cell_size, box, levels, min_score_ratio, max_nodes, batch):
        o = _capi.GlobalLocalizeOptions()
        self._lib.icpmi_global_localize_options_default(C.byref(o))
        o.cell_size, o.levels, o.min_score_ratio, o.max_nodes = float(cell_size), int(levels), float(min_score_ratio), int(max_nodes)
        if batch is not None:
            o.batch = int(batch)
        if box is not None:
            lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in box)
            o.has_box = 1
            o.box_lo[:], o.box_hi[:] = lo.tolist(), hi.tolist()
        return o

    def globalLocalize(self, reading, rotations, cell_size, box=None, levels=0, min_score_ratio=0.0, max_nodes=0, batch=None):
        """icpmi_global_localize: where is the sensor, with no candidate at all?  Exhaustive over the translations mu + cell_size * a of a
        lattice inside `box` ((lo, hi) in the map frame, metres; None: the map's bounding box) and the `rotations` ((K, 3, 3), K <= 4096;
        see yaw_rotations), by branch and bound over `levels` occupancy levels (0: automatic): the pose under which the most reading points
        fall into occupied cells of the map, exactly.  No normals, no matcher.  Returns a GlobalLocalization (found = False when nothing
        reaches min_score_ratio * N; proven = False when max_nodes stopped the search)."""
        scan = _f32c(reading, 4)
        R9 = self._rotations_to_c(rotations)
        o = self._global_localize_options(cell_size, box, levels, min_score_ratio, max_nodes, batch)
        res = _capi.GlobalLocalizeResult()
        self._check(self._lib.icpmi_global_localize(self._h, scan.ctypes.data, scan.shape[0], R9.ctypes.data, R9.shape[0] // 9, C.byref(o), C.byref(res)))
        return GlobalLocalization(res)

    def globalLocalizeDev(self, d_scan_ptr, n, rotations, cell_size, box=None, levels=0, min_score_ratio=0.0, max_nodes=0, batch=None):
        """icpmi_global_localize_dev: globalLocalize() for a reading already in HBM."""
        R9 = self._rotations_to_c(rotations)
        o = self._global_localize_options(cell_size, box, levels, min_score_ratio, max_nodes, batch)
        res = _capi.GlobalLocalizeResult()
        self._check(self._lib.icpmi_global_localize_dev(self._h, d_scan_ptr, int(n), R9.ctypes.data, R9.shape[0] // 9, C.byref(o), C.byref(res)))
        return GlobalLocalization(res)

    def occupancyScoreNodes(self, reading, rotations, cell_size, levels, nodes):
        """icpmi_occupancy_score_nodes (test seam and inspection): bound(k, l, A) of the (N, 5) `nodes` (k, l, A.x, A.y, A.z): (N,) int64"""
        scan = _f32c(reading, 4)
        R9 = self._rotations_to_c(rotations)
        nd = np.ascontiguousarray(np.asarray(nodes, dtype=np.int32).reshape(-1, 5))
        out = np.zeros(max(nd.shape[0], 1), dtype=np.int64)
        self._check(self._lib.icpmi_occupancy_score_nodes(self._h, scan.ctypes.data, scan.shape[0], R9.ctypes.data, R9.shape[0] // 9, float(cell_size),
                                                          int(levels), nd.ctypes.data, nd.shape[0], out.ctypes.data))
        return out[:nd.shape[0]]

    def occupancyLevel(self, cell_size, levels, level):
        """icpmi_get_occupancy_level: the cells of occB_level in ascending key order, (K, 3) int32"""
        nk = C.c_int64(0)
        self._check(self._lib.icpmi_get_occupancy_level(self._h, float(cell_size), int(levels), int(level), 0, None, C.byref(nk)))  # (a size query)
        ijk = np.zeros((max(nk.value, 1), 3), dtype=np.int32)
        self._check(self._lib.icpmi_get_occupancy_level(self._h, float(cell_size), int(levels), int(level), nk.value, ijk.ctypes.data, C.byref(nk)))
        return ijk[:nk.value]

    def occupancyInfo(self):
        """icpmi_get_occupancy_info: dict(levels, keys, bytes, build_ms (per level), builds) of the pyramid the handle holds"""
        lv, builds = C.c_int32(0), C.c_int64(0)
        keys, nbytes, ms = (C.c_int64 * 8)(), (C.c_int64 * 8)(), (C.c_float * 8)()
        self._check(self._lib.icpmi_get_occupancy_info(self._h, C.byref(lv), keys, nbytes, ms, C.byref(builds)))
        L = lv.value
        return dict(levels=L, keys=list(keys[:L]), bytes=list(nbytes[:L]), build_ms=list(ms[:L]), builds=builds.value)

    def relocalizeGlobal(self, reading, rotations, cell_size, normals=None, box=None, levels=0, min_score_ratio=0.0, max_nodes=0, **refine):
        """The search, then the existing refinement with the found pose as its one candidate: relocalize(reading, [pose], **refine), on a
        VoxelMatcher handle relocalizeVoxel(reading, normals, [pose], **refine).  Returns that call's Relocalization with the search's
        GlobalLocalization as `.search`; ConvergenceError when the search finds nothing."""
        found = self.globalLocalize(reading, rotations, cell_size, box=box, levels=levels, min_score_ratio=min_score_ratio, max_nodes=max_nodes)
        if not found.found:
            raise ConvergenceError("relocalizeGlobal: no pose reaches min_score_ratio")
        if self.getVoxelMatcher() > 0:
            if normals is None:
                raise InvalidField("relocalizeGlobal: a VoxelMatcher handle refines with the reading's normals")
            out = self.relocalizeVoxel(reading, normals, [found.pose], **refine)
        else:
            out = self.relocalize(reading, [found.pose], **refine)
        out.search = found
        return out

    def setReadingMaxDist(self, radii):
        """icpmi_set_reading_max_dist: the search radius of every point of the NEXT reading (KDTreeVarDistMatcher's `maxDistField` row; one shot)."""
        r = None if radii is None else np.ascontiguousarray(radii, dtype=np.float32).ravel()
        self._check(self._lib.icpmi_set_reading_max_dist(self._h, None if r is None else r.ctypes.data, 0 if r is None else r.shape[0]))

    def setReadingSensorNoise(self, noise):
        """icpmi_set_reading_sensor_noise: the `simpleSensorNoise` row of the NEXT reading (one shot; that call must bring scan_normals)."""
        nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32).ravel()
        self._check(self._lib.icpmi_set_reading_sensor_noise(self._h, None if nz is None else nz.ctypes.data, 0 if nz is None else nz.shape[0]))

    def setReadingScalar(self, scalar):
        """icpmi_set_reading_scalar: the descriptor row GenericDescriptorOutlierFilter{source: reading} reads, for the NEXT reading (one shot)."""
        sc = None if scalar is None else np.ascontiguousarray(scalar, dtype=np.float32).ravel()
        self._check(self._lib.icpmi_set_reading_scalar(self._h, None if sc is None else sc.ctypes.data, 0 if sc is None else sc.shape[0]))

    def registerDev(self, d_scan_ptr, n, fixed_iterations=0, d_normals_ptr=None):
        T = (C.c_float * 16)()
        self._last_n = int(n)
        if fixed_iterations > 0:
            st = self._lib.icpmi_register_fixed_dev(self._h, d_scan_ptr, n, d_normals_ptr, fixed_iterations, T, C.byref(self.stats))
        else:
            st = self._lib.icpmi_register_dev(self._h, d_scan_ptr, n, d_normals_ptr, T, C.byref(self.stats))
        self._check(st)
        return _T_from_c(T[:])

    def registerBatchDev(self, d_scan_ptrs, ns, fixed_iterations=0):
        """icpmi_register_batch_dev: B readings (device pointers, sizes) against the map in one launch sequence.
        Returns (list of 4x4 corrections, list of Stats, list of status codes)."""
        B = len(d_scan_ptrs)
        ptrs = (C.c_void_p * B)(*[int(p) for p in d_scan_ptrs])
        nn = (C.c_int64 * B)(*[int(n) for n in ns])
        T = (C.c_float * (16 * B))()
        stats = (_capi.Stats * B)()
        status = (C.c_int * B)()
        self._check(self._lib.icpmi_register_batch_dev(self._h, B, ptrs, nn, fixed_iterations, T, stats, status))
        self.batch_stats = stats
        return [_T_from_c(T[16 * b:16 * b + 16]) for b in range(B)], [stats[b] for b in range(B)], [int(status[b]) for b in range(B)]

    # ---- stage-level entry points ----
    def transform(self, T, cloud, normals=None):
        cloud = _f32c(cloud, 4)
        out = np.empty_like(cloud)
        Tc = _T_to_c(T)
        nin = nout = None
        outn = None
        if normals is not None:
            normals = _f32c(normals, 3)
            outn = np.empty_like(normals)
            nin, nout = normals.ctypes.data, outn.ctypes.data
        st = self._lib.icpmi_transform(self._h, Tc.ctypes.data_as(C.POINTER(C.c_float)), cloud.ctypes.data, cloud.shape[0],
                                       out.ctypes.data, nin, nout)
        if st == _capi.ERR_INVALID_ARG:
            raise TransformationError(self._lib.icpmi_last_error(self._h).decode())
        self._check(st)
        return (out, outn) if normals is not None else out

    def knn(self, queries_centred, k=1, max_dist=math.inf, allow_self=True):
        q = _f32c(queries_centred, 4)
        ids = np.empty((q.shape[0], k), dtype=np.int32)
        d2 = np.empty((q.shape[0], k), dtype=np.float32)
        self._check(self._lib.icpmi_knn(self._h, q.ctypes.data, q.shape[0], k, max_dist, int(allow_self), ids.ctypes.data, d2.ctypes.data))
        return ids, d2

    def knnVar(self, queries_centred, radii, k=1, allow_self=True):
        """icpmi_knn_var: knn with one search radius per query (KDTreeVarDistMatcher::findClosests)."""
        q = _f32c(queries_centred, 4)
        r = np.ascontiguousarray(radii, dtype=np.float32).ravel()
        if r.shape[0] != q.shape[0]:
            raise InvalidParameter("knnVar: one radius per query")
        ids = np.empty((q.shape[0], k), dtype=np.int32)
        d2 = np.empty((q.shape[0], k), dtype=np.float32)
        self._check(self._lib.icpmi_knn_var(self._h, q.ctypes.data, q.shape[0], k, r.ctypes.data, int(allow_self), ids.ctypes.data, d2.ctypes.data))
        return ids, d2

    def outlierWeights(self, d2, ids=None, read_normals=None):
        d2 = np.ascontiguousarray(d2, dtype=np.float32)
        n, k = d2.shape
        w = np.empty_like(d2)
        lim = C.c_float(-1)
        idp = None
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int32)
            idp = ids.ctypes.data
        rnp = None
        if read_normals is not None:
            read_normals = _f32c(read_normals, 3)
            rnp = read_normals.ctypes.data
        self._check(self._lib.icpmi_outlier_weights(self._h, d2.ctypes.data, idp, k, n, rnp, w.ctypes.data, C.byref(lim)))
        return w, float(lim.value)

    def minimizeStep(self, reading_centred, T_iter=None, read_normals=None):
        """icpmi_minimize_step; read_normals (N, 3): icpmi_minimize_step_normals (PlaneToPlaneErrorMinimizer, SurfaceNormalOutlierFilter)"""
        r = _f32c(reading_centred, 4)
        T = (C.c_float * 16)()
        sums = (C.c_double * 32)()
        tptr = None
        if T_iter is not None:
            Tc = _T_to_c(T_iter)
            tptr = Tc.ctypes.data
        if read_normals is not None:
            rn = _f32c(read_normals, 3)
            if rn.shape[0] != r.shape[0]:
                raise InvalidParameter("normals / cloud size mismatch")
            self._check(self._lib.icpmi_minimize_step_normals(self._h, r.ctypes.data, r.shape[0], rn.ctypes.data, tptr, T, sums, C.byref(self.stats)))
        else:
            self._check(self._lib.icpmi_minimize_step(self._h, r.ctypes.data, r.shape[0], tptr, T, sums, C.byref(self.stats)))
        return _T_from_c(T[:]), np.array(sums[:])

    def surfaceNormals(self, cloud, knn=5, with_densities=False, with_matched_ids=False, with_mean_dist=False):
        """normals [, densities] [, matched ids (m, knn) int32] [, mean distance (m,)] -- SurfaceNormalDataPointsFilter with
        keepDensities / keepMatchedIds / keepMeanDist."""
        c = _f32c(cloud, 4)
        out = np.empty((c.shape[0], 3), dtype=np.float32)
        if with_matched_ids or with_mean_dist:
            m = c.shape[0]
            dens = np.empty(m, dtype=np.float32) if with_densities else None
            ids = np.empty((m, knn), dtype=np.int32) if with_matched_ids else None
            md = np.empty(m, dtype=np.float32) if with_mean_dist else None
            ptr = lambda a: a.ctypes.data if a is not None else None
            self._check(self._lib.icpmi_surface_normals_ex2(self._h, c.ctypes.data, m, knn, out.ctypes.data, ptr(dens), ptr(ids), ptr(md)))
            return tuple(x for x in (out, dens, ids, md) if x is not None)
        if not with_densities:
            self._check(self._lib.icpmi_surface_normals(self._h, c.ctypes.data, c.shape[0], knn, out.ctypes.data))
            return out
        dens = np.empty(c.shape[0], dtype=np.float32)
        self._check(self._lib.icpmi_surface_normals_ex(self._h, c.ctypes.data, c.shape[0], knn, out.ctypes.data, dens.ctypes.data))
        return out, dens

    def surfaceNormalsEigen(self, cloud, knn=5):
        """(normals, eigenvalues (m, 3) ascending, eigenvectors (m, 9): entry 3 k + j = component k of eigenvector j) --
        SurfaceNormalDataPointsFilter with keepEigenValues / keepEigenVectors and sortEigen: 1 (icpmi_surface_normals_ex3)."""
        c = _f32c(cloud, 4); m = c.shape[0]
        out = np.empty((m, 3), dtype=np.float32); ev = np.empty((m, 3), dtype=np.float32); evec = np.empty((m, 9), dtype=np.float32)
        self._check(self._lib.icpmi_surface_normals_ex3(self._h, c.ctypes.data, m, knn, out.ctypes.data, None, None, None, ev.ctypes.data, evec.ctypes.data))
        return out, ev, evec

    def pointDistanceKeep(self, map_cloud, input_cloud, min_dist):
        m = _f32c(map_cloud, 4)
        i = _f32c(input_cloud, 4)
        keep = np.empty(i.shape[0], dtype=np.uint8)
        self._check(self._lib.icpmi_point_distance_keep(self._h, m.ctypes.data, m.shape[0], i.ctypes.data, i.shape[0], min_dist, keep.ctypes.data))
        return keep.astype(bool)

    def voxelKeepFirst(self, cloud, edge):
        """Lattice stand-in of OctreeGridDataPointsFilter{maxSizeByNode: edge, samplingMethod: 0}
        (OctreeMapperModule.cpp:35-39): mask of the first point of every occupied voxel."""
        c = _f32c(cloud, 4)
        keep = np.empty(c.shape[0], dtype=np.uint8)
        self._check(self._lib.icpmi_voxel_keep_first(self._h, c.ctypes.data, c.shape[0], edge, keep.ctypes.data))
        return keep.astype(bool)

    def filterPoints(self, cloud, filters):
        """Mapper::applyInputFilters as one pass: filters = [("distance_limit", dim, dist, remove_inside) |
        ("bounding_box", (xmin, ymin, zmin), (xmax, ymax, zmax), remove_inside)]; returns the keep mask."""
        from . import _capi
        c = _f32c(cloud, 4)
        arr = (_capi.PointFilter * max(1, len(filters)))()
        for k, flt in enumerate(filters):
            if flt[0] == "distance_limit":
                arr[k].type = 0; arr[k].i = int(flt[1]); arr[k].f[0] = flt[2]; arr[k].f[1] = 1.0 if flt[3] else 0.0
            elif flt[0] == "bounding_box":
                arr[k].type = 1; arr[k].i = 1 if flt[3] else 0
                for r in range(3):
                    arr[k].f[r] = flt[1][r]; arr[k].f[3 + r] = flt[2][r]
            else:
                raise InvalidParameter("unknown point filter " + str(flt[0]))
        keep = np.empty(c.shape[0], dtype=np.uint8)
        self._check(self._lib.icpmi_filter_points(self._h, c.ctypes.data, c.shape[0], arr, len(filters), keep.ctypes.data))
        return keep.astype(bool)

    def samplingSurfaceNormal(self, cloud, ratio=0.5, knn=7, max_box_dim=math.inf, seed=1):
        """icpmi_sampling_surface_normal: (kept indices in box order, their normals) -- SamplingSurfaceNormalDataPointsFilter, samplingMethod 0."""
        c = _f32c(cloud, 4)
        order = np.empty(c.shape[0], dtype=np.int32)
        nrm = np.empty((c.shape[0], 3), dtype=np.float32)
        n_out = C.c_int64(0)
        self._check(self._lib.icpmi_sampling_surface_normal(self._h, c.ctypes.data, c.shape[0], ratio, knn, max_box_dim, seed, order.ctypes.data,
                                                            nrm.ctypes.data, C.byref(n_out)))
        return order[:n_out.value].copy(), nrm[:n_out.value].copy()

    def samplingSurfaceNormalBoxes(self, cloud, knn=7, max_box_dim=math.inf):
        """icpmi_sampling_surface_normal_ex with samplingMethod 1: one point per surviving box -- (first member index, normal, mean of the box,
        member start, member count, members in index order)."""
        c = _f32c(cloud, 4); n = c.shape[0]
        order = np.empty(n, dtype=np.int32); nrm = np.empty((n, 3), dtype=np.float32); mean = np.empty((n, 3), dtype=np.float32)
        ms = np.empty(n, dtype=np.int32); mc = np.empty(n, dtype=np.int32); mem = np.empty(n, dtype=np.int32)
        n_out = C.c_int64(0)
        self._check(self._lib.icpmi_sampling_surface_normal_ex(self._h, c.ctypes.data, n, 1.0, knn, max_box_dim, 1, 1, order.ctypes.data, nrm.ctypes.data,
                                                               C.byref(n_out), mean.ctypes.data, ms.ctypes.data, mc.ctypes.data, mem.ctypes.data))
        k = n_out.value
        tot = int(ms[k - 1] + mc[k - 1]) if k else 0
        return order[:k].copy(), nrm[:k].copy(), mean[:k].copy(), ms[:k].copy(), mc[:k].copy(), mem[:tot].copy()

    def octreeSample(self, cloud, max_size, max_points=1, method=0, with_leaves=False):
        """OctreeGridDataPointsFilter: indices of the kept points in leaf-visiting order (+ the leaf ordinal of every point)"""
        c = _f32c(cloud, 4)
        order = np.empty(c.shape[0], dtype=np.int32)
        leaf = np.empty(c.shape[0], dtype=np.int32) if with_leaves else None
        m = C.c_int64(0)
        self._check(self._lib.icpmi_octree_sample(self._h, c.ctypes.data, c.shape[0], max_size, max_points, method, order.ctypes.data,
                                                  None if leaf is None else leaf.ctypes.data, C.byref(m)))
        return (order[:m.value].copy(), leaf) if with_leaves else order[:m.value].copy()

    def voxelGrid(self, cloud, vsize, average_descriptors=True, descriptors=None):
        """VoxelGridDataPointsFilter (useCentroid: 1; the formulation of icpmi_voxel_grid, as recalled): vsize = one edge or
        (vSizeX, vSizeY, vSizeZ); descriptors = (N, rows) or (N,) point-major, or None.  Returns (order, out4, desc_out):
        the first-point index of every voxel in ascending order, the centroids (N', 4) and the descriptor rows (N', rows)
        -- averaged, or the first point's when average_descriptors is False -- or None without descriptors."""
        c = _f32c(cloud, 4)
        n = c.shape[0]
        vs = np.broadcast_to(np.asarray(vsize, dtype=np.float32), (3,)).copy()
        d = None
        rows = 0
        if descriptors is not None:
            d = np.ascontiguousarray(descriptors, dtype=np.float32)
            d = d.reshape(n, 1) if d.ndim == 1 else d
            if d.ndim != 2 or d.shape[0] != n:
                raise InvalidParameter(f"descriptors must be ({n}, rows), got {d.shape}")
            rows = d.shape[1]
        order = np.empty(n, dtype=np.int32)
        out4 = np.empty((n, 4), dtype=np.float32)
        dout = np.empty((n, rows), dtype=np.float32) if d is not None else None
        m = C.c_int64(0)
        self._check(self._lib.icpmi_voxel_grid(self._h, c.ctypes.data, n, vs.ctypes.data, 1 if average_descriptors else 0,
                                               None if d is None else d.ctypes.data, rows, order.ctypes.data, out4.ctypes.data,
                                               None if dout is None else dout.ctypes.data, C.byref(m)))
        k = m.value
        return order[:k].copy(), out4[:k].copy(), (None if dout is None else dout[:k].copy())

    def covarianceSampling(self, cloud, normals, nb_sample=5000, torque_norm=1, with_info=False):
        """CovarianceSamplingDataPointsFilter{nbSample, torqueNorm} (the formulation of icpmi_covariance_sampling, as recalled):
        cloud (N, 4), normals (N, 3) or None.  Returns the selected indices in selection order (int32), or (order, info) with info
        = {center (3,), lnorm, eigval (6,) ascending, basis (6, 6), column k = x_k} -- None when nb_sample >= N (nothing sampled)."""
        c = _f32c(cloud, 4)
        n = c.shape[0]
        nptr = None
        if normals is not None:
            normals = _f32c(normals, 3)
            if normals.shape[0] != n:
                raise InvalidParameter("normals / cloud size mismatch")
            nptr = normals.ctypes.data
        order = np.empty(max(0, min(n, int(nb_sample))), dtype=np.int32)
        info = _capi.CovSampInfo()
        m = C.c_int64(0)
        self._check(self._lib.icpmi_covariance_sampling(self._h, c.ctypes.data, n, nptr, int(nb_sample), int(torque_norm), order.ctypes.data,
                                                        C.byref(m), C.byref(info)))
        order = order[:m.value].copy()
        if not with_info:
            return order
        if nb_sample >= n:
            return order, None
        return order, {"center": np.array(info.center[:]), "lnorm": float(info.lnorm), "eigval": np.array(info.eigval[:]),
                       "basis": np.array(info.basis[:]).reshape(6, 6).T.copy()}

    def sensorModel(self, cloud, steps, normals=None, obs_dirs=None):
        """icpmi_sensor_model: a run of the four sensor-model DataPointsFilters as one pass.  steps = [("observation_direction", x, y, z) |
        ("orient_normals", toward_center) | ("shadow", eps) | ("simple_sensor_noise", sensor_type, gain)], at most 8, in chain order;
        cloud (N, 4), normals / obs_dirs (N, 3) or None.  Returns a dict with what the program produced: "normals" (N, 3) after
        orient_normals, "observationDirections" (N, 3) after observation_direction, "simpleSensorNoise" (N,) after simple_sensor_noise,
        "keep" (N,) bool after shadow.  Rows are NOT compacted: apply "keep" to every row, as the host shell does."""
        c = _f32c(cloud, 4)
        n = c.shape[0]
        arr = (_capi.SensorStep * max(1, len(steps)))()
        kinds = set()
        for k, st in enumerate(steps):
            kinds.add(st[0])
            if st[0] == "observation_direction":
                arr[k].type = _capi.SM_OBSERVATION_DIRECTION
                for r in range(3):
                    arr[k].f[r] = st[1 + r]
            elif st[0] == "orient_normals":
                arr[k].type = _capi.SM_ORIENT_NORMALS; arr[k].i = 1 if (st[1] if len(st) > 1 else 1) else 0
            elif st[0] == "shadow":
                arr[k].type = _capi.SM_SHADOW; arr[k].f[0] = st[1] if len(st) > 1 else 0.1
            elif st[0] == "simple_sensor_noise":
                arr[k].type = _capi.SM_SIMPLE_SENSOR_NOISE; arr[k].i = int(st[1]) if len(st) > 1 else 0
                arr[k].f[0] = st[2] if len(st) > 2 else 1.0
            else:
                raise InvalidParameter("unknown sensor-model step " + str(st[0]))

        def _in3(a, what):
            if a is None:
                return None
            a = _f32c(a, 3)
            if a.shape[0] != n:
                raise InvalidParameter(what + " / cloud size mismatch")
            return a
        nrm, od = _in3(normals, "normals"), _in3(obs_dirs, "obs_dirs")
        out = {}
        if "orient_normals" in kinds:
            out["normals"] = np.empty((n, 3), dtype=np.float32)
        if "observation_direction" in kinds:
            out["observationDirections"] = np.empty((n, 3), dtype=np.float32)
        if "simple_sensor_noise" in kinds:
            out["simpleSensorNoise"] = np.empty(n, dtype=np.float32)
        if "shadow" in kinds:
            out["keep"] = np.empty(n, dtype=np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data
        st = self._lib.icpmi_sensor_model(self._h, c.ctypes.data, n, ptr(nrm), ptr(od), arr, len(steps), ptr(out.get("normals")),
                                          ptr(out.get("observationDirections")), ptr(out.get("simpleSensorNoise")), ptr(out.get("keep")))
        if st == _capi.ERR_INVALID_ARG:  # a missing descriptor is upstream's InvalidField, whatever the status it travels under
            msg = self._lib.icpmi_last_error(self._h).decode()
            if msg.startswith("InvalidField"):
                raise InvalidField(msg)
        self._check(st)
        if "keep" in out:
            out["keep"] = out["keep"].astype(bool)
        return out

    @staticmethod
    def _sweepMotion(stamps, poses, ref, unit, round, extrapolate):
        """(icpmi_sweep_motion, the arrays it points into): stamps (K,) seconds from the scan's stamp, poses (K, 7) tx ty tz qx qy qz qw"""
        s = np.ascontiguousarray(stamps, dtype=np.float64).ravel()
        p = np.ascontiguousarray(poses, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 7 or p.shape[0] != s.shape[0]:
            raise InvalidParameter(f"expected {s.shape[0]} poses as a (K, 7) array (tx ty tz qx qy qz qw), got {p.shape}")
        m = _capi.SweepMotion(n_poses=s.shape[0], extrapolate=1 if extrapolate else 0, stamp_s=s.ctypes.data_as(C.POINTER(C.c_double)),
                              pose7=p.ctypes.data_as(C.POINTER(C.c_double)), ref_s=float(ref), time_unit_s=float(unit), round_s=float(round))
        return m, (s, p)

    def deskew(self, points, t_rel, stamps, poses, ref=0.0, unit=1e-9, round=0.0, extrapolate=False, normals=None):
        """icpmi_deskew: motion compensation of one sweep.  points (N, 4); t_rel (N,) the points' times in units of `unit` seconds from
        the scan's stamp; stamps (K,) seconds from the scan's stamp and poses (K, 7) (tx ty tz qx qy qz qw) the sensor's motion; the
        output is expressed at time `ref`.  round > 0 rounds the point times to multiples of it (seconds) first; extrapolate clamps
        times outside the table instead of failing.  Returns the deskewed cloud, or (cloud, normals) when normals (N, 3) are given."""
        c = _f32c(points, 4)
        n = c.shape[0]
        t = np.ascontiguousarray(t_rel, dtype=np.float32).ravel()
        if t.shape[0] != n:
            raise InvalidParameter("t_rel / cloud size mismatch")
        m, keep = self._sweepMotion(stamps, poses, ref, unit, round, extrapolate)
        out = np.empty_like(c)
        nin = nout = outn = None
        if normals is not None:
            normals = _f32c(normals, 3)
            if normals.shape[0] != n:
                raise InvalidParameter("normals / cloud size mismatch")
            outn = np.empty_like(normals)
            nin, nout = normals.ctypes.data, outn.ctypes.data
        self._check(self._lib.icpmi_deskew(self._h, c.ctypes.data, n, t.ctypes.data, C.byref(m), out.ctypes.data, nin, nout))
        return (out, outn) if normals is not None else out

    def deskewDev(self, d_points_ptr, n, d_t_rel_ptr, stamps, poses, ref=0.0, unit=1e-9, round=0.0, extrapolate=False, d_out_ptr=None,
                  d_normals_ptr=None, d_normals_out_ptr=None):
        """icpmi_deskew_dev: the same on device pointers, on the handle's stream; in place unless d_out_ptr / d_normals_out_ptr are given."""
        m, keep = self._sweepMotion(stamps, poses, ref, unit, round, extrapolate)
        if d_normals_ptr is not None and d_normals_out_ptr is None:
            d_normals_out_ptr = d_normals_ptr
        self._check(self._lib.icpmi_deskew_dev(self._h, d_points_ptr, int(n), d_t_rel_ptr, C.byref(m), d_points_ptr if d_out_ptr is None else d_out_ptr,
                                               d_normals_ptr, d_normals_out_ptr))

    # ---- sweep registration: the motion within one scan estimated by ICP (icpmi_register_sweep*, icpmi_sweep_sums, icpmi_sweep_solve) ----
    def _sweepOptions(self, begin, end, unit, max_iterations, min_step_rot, min_step_trans, lambda_rot, lambda_trans):
        o = _capi.SweepOptions()
        self._lib.icpmi_sweep_options_default(C.byref(o))
        o.begin_s, o.end_s, o.time_unit_s = float(begin), float(end), float(unit)
        o.max_iterations = int(max_iterations)
        o.min_step_rot = -1.0 if min_step_rot is None else float(min_step_rot)
        o.min_step_trans = -1.0 if min_step_trans is None else float(min_step_trans)
        o.lambda_rot, o.lambda_trans = float(lambda_rot), float(lambda_trans)
        return o

    def _sweep_out(self, st):
        if st == _capi.ERR_INVALID_ARG:
            msg = self._lib.icpmi_last_error(self._h).decode()
            if msg.startswith("TransformationError"):
                raise TransformationError(msg)
        self._check(st)

    def register_sweep(self, scan, t_rel, prior_begin, prior_end, begin=0.0, end=0.1, unit=1e-9, max_iterations=12, min_step_rot=None,
                       min_step_trans=None, lambda_rot=0.0, lambda_trans=0.0, with_cloud=False):
        """icpmi_register_sweep: scan (N, 4) in the sensor frame as measured (skewed), t_rel (N,) the points' times in units of `unit`
        seconds from the scan's stamp, the sweep spanning [begin, end] seconds; prior_begin / prior_end: 4 x 4 guesses of the sensor's
        pose in the map at the two ends.  Returns a SweepResult (T_begin, T_end, pose7 (2, 7), iterations, stop_reason, pairs, weight_sum,
        sum_sq, weighted_point_used_ratio, trimmed_limit), or (result, cloud) with the scan deskewed to the end pose when with_cloud."""
        c = _f32c(scan, 4)
        n = c.shape[0]
        t = np.ascontiguousarray(t_rel, dtype=np.float32).ravel()
        if t.shape[0] != n:
            raise InvalidParameter("t_rel / cloud size mismatch")
        o = self._sweepOptions(begin, end, unit, max_iterations, min_step_rot, min_step_trans, lambda_rot, lambda_trans)
        res = _capi.SweepResult()
        out = np.empty_like(c) if with_cloud else None
        Tb, Te = _T_to_c(prior_begin), _T_to_c(prior_end)
        self._sweep_out(self._lib.icpmi_register_sweep(self._h, c.ctypes.data, n, t.ctypes.data, Tb.ctypes.data, Te.ctypes.data, C.byref(o),
                                                       C.byref(res), None if out is None else out.ctypes.data))
        r = SweepResult(res)
        return (r, out) if with_cloud else r

    def register_sweep_dev(self, d_scan_ptr, n, d_t_rel_ptr, prior_begin, prior_end, begin=0.0, end=0.1, unit=1e-9, max_iterations=12,
                           min_step_rot=None, min_step_trans=None, lambda_rot=0.0, lambda_trans=0.0, d_out_ptr=None):
        """icpmi_register_sweep_dev: register_sweep on device pointers, on the handle's stream; d_out_ptr (not the scan) receives the cloud."""
        o = self._sweepOptions(begin, end, unit, max_iterations, min_step_rot, min_step_trans, lambda_rot, lambda_trans)
        res = _capi.SweepResult()
        Tb, Te = _T_to_c(prior_begin), _T_to_c(prior_end)
        self._sweep_out(self._lib.icpmi_register_sweep_dev(self._h, d_scan_ptr, int(n), d_t_rel_ptr, Tb.ctypes.data, Te.ctypes.data, C.byref(o),
                                                           C.byref(res), d_out_ptr))
        return SweepResult(res)

    def sweep_sums(self, scan, t_rel, T_begin, T_end, begin=0.0, end=0.1, unit=1e-9):
        """icpmi_sweep_sums: one pass (deskew, match, select, pair sums) under the given poses.  Returns (sums (80,) float64, SweepResult)."""
        c = _f32c(scan, 4)
        n = c.shape[0]
        t = np.ascontiguousarray(t_rel, dtype=np.float32).ravel()
        if t.shape[0] != n:
            raise InvalidParameter("t_rel / cloud size mismatch")
        o = self._sweepOptions(begin, end, unit, 1, None, None, 0.0, 0.0)
        res = _capi.SweepResult()
        sums = np.zeros(80, dtype=np.float64)
        Tb, Te = _T_to_c(T_begin), _T_to_c(T_end)
        self._sweep_out(self._lib.icpmi_sweep_sums(self._h, c.ctypes.data, n, t.ctypes.data, Tb.ctypes.data, Te.ctypes.data, C.byref(o),
                                                   sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(res)))
        return sums, SweepResult(res)

    @staticmethod
    def sweep_solve(sums, lambda_rot=0.0, lambda_trans=0.0, d=None):
        """icpmi_sweep_solve (host only, no handle): the step x = (xi_b, xi_e) (12,) float64 of the system in sums (80,)."""
        return sweep_solve(sums, lambda_rot, lambda_trans, d)

    def normalSpaceSampling(self, cloud, normals, nb_sample=5000, seed=1, epsilon=0.09817, with_buckets=False):
        """NormalSpaceDataPointsFilter{nbSample, seed, epsilon} (the formulation of icpmi_normal_space_sampling, as recalled): cloud
        (N, 4), normals (N, 3) or None.  Returns the kept indices in ascending order (int32), or (order, buckets) with buckets (N,)
        int32 = the device's angular bucket of every point -- None when nb_sample >= N or nb_sample == 0 (nothing sampled)."""
        c = _f32c(cloud, 4)
        n = c.shape[0]
        nptr = None
        if normals is not None:
            normals = _f32c(normals, 3)
            if normals.shape[0] != n:
                raise InvalidParameter("normals / cloud size mismatch")
            nptr = normals.ctypes.data
        order = np.empty(max(0, min(n, int(nb_sample))), dtype=np.int32)
        buckets = np.empty(n, dtype=np.int32) if with_buckets else None
        m = C.c_int64(0)
        self._check(self._lib.icpmi_normal_space_sampling(self._h, c.ctypes.data, n, nptr, int(nb_sample), int(seed), float(epsilon),
                                                          order.ctypes.data, C.byref(m), None if buckets is None else buckets.ctypes.data))
        order = order[:m.value].copy()
        if not with_buckets:
            return order
        return order, (None if nb_sample >= n or nb_sample == 0 else buckets)

    def maxDensityKeep(self, densities, max_density=10.0, seed=1):
        """MaxDensityDataPointsFilter{maxDensity, seed} (the formulation of icpmi_max_density_keep): densities (N,) -> bool keep mask."""
        d = np.ascontiguousarray(densities, dtype=np.float32)
        keep = np.empty(d.shape[0], dtype=np.uint8)
        self._check(self._lib.icpmi_max_density_keep(self._h, d.ctypes.data, d.shape[0], float(max_density), int(seed), keep.ctypes.data))
        return keep.astype(bool)

    def voxelKeep(self, cloud, edge, method=0):
        """Same lattice, representative by `samplingMethod`: 0 first point, 1 pseudo-random point (smallest fmix32 of the index)."""
        c = _f32c(cloud, 4)
        keep = np.empty(c.shape[0], dtype=np.uint8)
        self._check(self._lib.icpmi_voxel_keep(self._h, c.ctypes.data, c.shape[0], edge, method, keep.ctypes.data))
        return keep.astype(bool)

    @staticmethod
    def _mapOps(modules, post):
        """[(name, params...)] -> MapOp array.  Names: 'point_distance' (min_dist), 'dynamic_points' (7 parameters in
        icpmi_dynpts_params order), 'voxel' (edge, method), 'surface_normals' (knn, keep_densities = 0), 'cut_scalar' (threshold,
        use_larger_than), 'max_density' (max_density, seed = 1)."""
        from . import _capi
        ops = (_capi.MapOp * (len(modules) + len(post)))()
        for j, item in enumerate(list(modules) + list(post)):
            name, args = item[0], item[1:]
            op = ops[j]
            if name == "point_distance":
                op.type = _capi.MOP_POINT_DISTANCE; op.f[0] = args[0]
            elif name == "dynamic_points":
                op.type = _capi.MOP_DYNAMIC_POINTS
                for r in range(7):
                    op.f[r] = args[r]
            elif name == "voxel":
                op.type = _capi.MOP_VOXEL; op.f[0] = args[0]; op.i = int(args[1]) if len(args) > 1 else 0
            elif name == "octree":      # (maxSizeByNode, samplingMethod = 0, maxPointByNode = 1)
                op.type = _capi.MOP_OCTREE; op.f[0] = args[0]; op.i = int(args[1]) if len(args) > 1 else 0
                op.f[1] = float(args[2]) if len(args) > 2 else 1.0
            elif name == "surface_normals":
                op.type = _capi.MOP_SURFACE_NORMALS; op.i = int(args[0]); op.f[0] = 1.0 if len(args) > 1 and args[1] else 0.0
            elif name == "cut_scalar":
                op.type = _capi.MOP_CUT_SCALAR; op.f[0] = args[0]; op.i = int(args[1]) if len(args) > 1 else 1
            elif name == "max_density":
                op.type = _capi.MOP_MAX_DENSITY; op.f[0] = args[0]; op.i = int(args[1]) if len(args) > 1 else 1
            else:
                raise InvalidParameter("unknown map operator " + name)
        return ops

    def mapUpdateChain(self, scan_in_map_frame, modules, post=(), scan_scalar=None, scan_normals=None, to_sensor=None, staged_correction=None,
                       with_prefix=False, want_src=True, from_sensor=None):
        """Map::updateLocalPointCloud (Map.cpp:502-534) for a whole module chain + post filters on the resident map.
        Returns (src, m): new map point j was point src[j] of [old map ; scan].  With staged_correction the scan is the
        one staged by registerWithPrior (scan_in_map_frame is ignored)."""
        ops = self._mapOps(modules, post)
        m_old = C.c_int64(0)
        self._check(self._lib.icpmi_get_map(self._h, None, None, 0, C.byref(m_old)))
        ss = None if scan_scalar is None else np.ascontiguousarray(scan_scalar, dtype=np.float32)
        Ts = None if to_sensor is None else _T_to_c(to_sensor)
        Tf = None if from_sensor is None else _T_to_c(from_sensor)   # pose: the post filters then run in the sensor frame (Map.cpp:523-525)
        Tfp = None if Tf is None else Tf.ctypes.data
        new_m = C.c_int64(0)
        head = C.c_int64(0)
        hp = C.byref(head) if with_prefix else None
        if not want_src:   # a caller without further descriptors does not need the provenance vector (3 MB per update at 800 k points)
            Tc = None if staged_correction is None else _T_to_c(staged_correction)
            if staged_correction is not None:
                self._check(self._lib.icpmi_map_update_chain_staged(self._h, Tc.ctypes.data, None if ss is None else ss.ctypes.data,
                                                                    None if Ts is None else Ts.ctypes.data, Tfp, ops, len(ops), len(modules),
                                                                    None, 0, None, C.byref(new_m)))
            else:
                sc = _f32c(scan_in_map_frame, 4)
                sn = None if scan_normals is None else _f32c(scan_normals, 3)
                self._check(self._lib.icpmi_map_update_chain(self._h, sc.ctypes.data, sc.shape[0], None if sn is None else sn.ctypes.data,
                                                             None if ss is None else ss.ctypes.data, None if Ts is None else Ts.ctypes.data, Tfp,
                                                             ops, len(ops), len(modules), None, 0, None, C.byref(new_m)))
            return None, int(new_m.value)
        if staged_correction is not None:
            n = self._staged_n
            src = np.empty(m_old.value + max(1, len(modules)) * n + 1, dtype=np.int32)
            Tc = _T_to_c(staged_correction)
            self._check(self._lib.icpmi_map_update_chain_staged(self._h, Tc.ctypes.data, None if ss is None else ss.ctypes.data,
                                                                None if Ts is None else Ts.ctypes.data, Tfp, ops, len(ops), len(modules),
                                                                src.ctypes.data, src.shape[0], hp, C.byref(new_m)))
        else:
            sc = _f32c(scan_in_map_frame, 4)
            sn = None if scan_normals is None else _f32c(scan_normals, 3)
            n = sc.shape[0]
            src = np.empty(m_old.value + max(1, len(modules)) * n + 1, dtype=np.int32)
            self._check(self._lib.icpmi_map_update_chain(self._h, sc.ctypes.data, n, None if sn is None else sn.ctypes.data,
                                                         None if ss is None else ss.ctypes.data, None if Ts is None else Ts.ctypes.data, Tfp,
                                                         ops, len(ops), len(modules), src.ctypes.data, src.shape[0], hp, C.byref(new_m)))
        if with_prefix:  # the head was not written by the library: it is the identity
            src[:head.value] = np.arange(head.value, dtype=np.int32)
            return src[:new_m.value].copy(), int(new_m.value), int(head.value)
        return src[:new_m.value].copy(), int(new_m.value)

    def setMapScalar(self, scalar):
        s = np.ascontiguousarray(scalar, dtype=np.float32)
        self._check(self._lib.icpmi_set_map_scalar(self._h, s.ctypes.data, s.shape[0]))

    def getMapScalar(self):
        m = C.c_int64(0)
        self._check(self._lib.icpmi_get_map(self._h, None, None, 0, C.byref(m)))
        out = np.empty(m.value, dtype=np.float32)
        self._check(self._lib.icpmi_get_map_scalar(self._h, out.ctypes.data, out.shape[0]))
        return out

    def getMapDensities(self):
        """The `densities` row of the resident map (a 'surface_normals' step with keep_densities wrote it), or None when it has none.
        icpmi_get_map_densities writes nothing without a valid row: the buffer goes in filled with a NaN payload no density can have."""
        m = C.c_int64(0)
        self._check(self._lib.icpmi_get_map(self._h, None, None, 0, C.byref(m)))
        if m.value == 0:
            return None
        bits = np.full(m.value, 0x7FC0DE05, dtype=np.uint32)
        self._check(self._lib.icpmi_get_map_densities(self._h, bits.ctypes.data, bits.shape[0]))
        return None if (bits == 0x7FC0DE05).all() else bits.view(np.float32)

    def dynamicPointsUpdate(self, to_sensor, input_cloud, map_cloud, map_normals, prob_dynamic, threshold_dynamic=0.6, alpha=0.8,
                            beta=0.99, beam_half_angle=0.01, epsilon_a=0.01, epsilon_d=0.01, sensor_max_range=200.0):
        """DynamicPointsMapperModule::inPlaceUpdateMap (DynamicPointsMapperModule.cpp:34-172): returns the
        updated `probabilityDynamic` of the map.  `to_sensor` = pose^-1 (row-major 4x4 numpy)."""
        prm = np.array([threshold_dynamic, alpha, beta, beam_half_angle, epsilon_a, epsilon_d, sensor_max_range], dtype=np.float32)
        T = _T_to_c(to_sensor)
        i = _f32c(input_cloud, 4); m = _f32c(map_cloud, 4); nn = _f32c(map_normals, 3)
        out = np.ascontiguousarray(prob_dynamic, dtype=np.float32).copy()
        if out.shape[0] != m.shape[0] or nn.shape[0] != m.shape[0]:
            raise InvalidParameter("dynamicPointsUpdate: map, normals and probabilities must have the same length")
        self._check(self._lib.icpmi_dynamic_points_update(self._h, prm.ctypes.data, T.ctypes.data,
                                                          i.ctypes.data, i.shape[0], m.ctypes.data, nn.ctypes.data, m.shape[0], out.ctypes.data))
        return out

    def mapUpdatePointDistance(self, scan_in_map_frame, min_dist, normals_knn=0, scan_normals=None, return_keep=False):
        """Map::updateLocalPointCloud for the PointDistance chain on the resident map (Map.cpp:502-534): returns
        (points appended, points in the map afterwards[, keep mask]).  Only the scan is uploaded."""
        sc = _f32c(scan_in_map_frame, 4)
        sn = None if scan_normals is None else _f32c(scan_normals, 3)
        app = C.c_int64(0); m = C.c_int64(0)
        keep = np.zeros(sc.shape[0], dtype=np.uint8) if return_keep else None
        self._check(self._lib.icpmi_map_update_point_distance(self._h, sc.ctypes.data, sc.shape[0], None if sn is None else sn.ctypes.data,
                                                              min_dist, normals_knn, None if keep is None else keep.ctypes.data,
                                                              C.byref(app), C.byref(m)))
        return (int(app.value), int(m.value), keep.astype(bool)) if return_keep else (int(app.value), int(m.value))

    def registerWithPrior(self, scan_sensor_frame, prior):
        """Mapper::processInput's first half with the scan staged once (Mapper.cpp:197,213): the scan goes into the map
        frame by `prior` on the device, is registered, and stays in HBM for mapUpdateStaged.  Returns the correction."""
        sc = _f32c(scan_sensor_frame, 4)
        P = _T_to_c(prior)
        T = (C.c_float * 16)()
        self._check(self._lib.icpmi_register_prior(self._h, sc.ctypes.data, sc.shape[0], P.ctypes.data, T, C.byref(self.stats)))
        self._staged_n = self._last_n = sc.shape[0]
        return _T_from_c(T[:])

    def registerWithPriorDev(self, d_scan_ptr, n, prior):
        """icpmi_register_prior_dev: registerWithPrior for a sensor-frame scan that is already in HBM."""
        P = _T_to_c(prior)
        T = (C.c_float * 16)()
        self._check(self._lib.icpmi_register_prior_dev(self._h, d_scan_ptr, n, P.ctypes.data, T, C.byref(self.stats)))
        self._staged_n = self._last_n = n
        return _T_from_c(T[:])

    def mapUpdateStaged(self, correction, min_dist, normals_knn=0, return_keep=False):
        """Second half (Mapper.cpp:221 + Map::updateLocalPointCloud): the staged cloud moved by `correction`, then the
        PointDistance update on the resident map."""
        Tc = _T_to_c(correction)
        app = C.c_int64(0); m = C.c_int64(0)
        n = C.c_int64(0)
        keep = None
        if return_keep:
            # the staged scan's size is the size of the last registerWithPrior reading
            keep = np.zeros(self._staged_n, dtype=np.uint8)
        self._check(self._lib.icpmi_map_update_staged(self._h, Tc.ctypes.data, min_dist, normals_knn, None if keep is None else keep.ctypes.data,
                                                      C.byref(app), C.byref(m)))
        return (int(app.value), int(m.value), keep.astype(bool)) if return_keep else (int(app.value), int(m.value))

    def stagedPointDistanceKeep(self, correction, min_dist):
        """Keep mask of the staged scan (moved by `correction`) against the resident map, map untouched; returns
        (mask, moved cloud).  The scan-sharded loop exchanges the accepted points before any replica appends them."""
        Tc = _T_to_c(correction)
        keep = np.zeros(self._staged_n, dtype=np.uint8)
        placed = np.empty((self._staged_n, 4), dtype=np.float32)
        self._check(self._lib.icpmi_staged_point_distance_keep(self._h, Tc.ctypes.data, min_dist, keep.ctypes.data, placed.ctypes.data))
        return keep.astype(bool), placed

    # ---- scan-sharded mapping: RCCL communicator + device-resident map-growth epoch ----
    @staticmethod
    def commUniqueId():
        """rank 0: a fresh communicator id (128 bytes) to hand to the other ranks"""
        lib = _capi.load()
        buf = (C.c_char * 128)()
        st = lib.icpmi_comm_get_unique_id(buf)
        if st != _capi.ICPMI_OK:
            raise HipError(lib.icpmi_last_error(None).decode())
        return bytes(buf)

    def commInit(self, unique_id, n_ranks, rank):
        buf = (C.c_char * 128).from_buffer_copy(unique_id)
        self._check(self._lib.icpmi_comm_init(self._h, buf, n_ranks, rank))

    def commInfo(self):
        """icpmi_comm_info: (ranks, rank, kind) as the communicator itself reports them; kind 0 none / 1 RCCL / 2 loopback."""
        a, b, k = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.icpmi_comm_info(self._h, C.byref(a), C.byref(b), C.byref(k)))
        return int(a.value), int(b.value), int(k.value)

    def commDestroy(self):
        self._check(self._lib.icpmi_comm_destroy(self._h))

    def stagedMergeAllGather(self, correction, min_dist, normals_knn=0, return_merged=False, merged_capacity=None):
        """icpmi_staged_merge_allgather: (accepted on this rank, appended on every replica, new map size[, merged points]).
        correction None: this rank contributes nothing (empty scan / failed registration) and still takes part in the exchange.
        The merged set is fetched with icpmi_staged_merged_points once its size is known (merged_capacity only sizes the
        optional in-call copy, which may be smaller than the set)."""
        Tc = None if correction is None else _T_to_c(correction)
        acc, app, new_m, mn = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        out = None
        if return_merged and merged_capacity is not None:
            out = np.empty((int(merged_capacity), 4), dtype=np.float32)
        self._check(self._lib.icpmi_staged_merge_allgather(self._h, None if Tc is None else Tc.ctypes.data, min_dist, normals_knn, C.byref(acc),
                                                           C.byref(app), C.byref(new_m), None if out is None else out.ctypes.data,
                                                           0 if out is None else out.shape[0], C.byref(mn)))
        if return_merged:
            if out is None or mn.value > out.shape[0]:
                out = self.stagedMergedPoints()
            return int(acc.value), int(app.value), int(new_m.value), out[:mn.value].copy()
        return int(acc.value), int(app.value), int(new_m.value)

    def stagedMergedPoints(self):
        """icpmi_staged_merged_points: the merged set of the last epoch."""
        n = C.c_int64(0)
        self._check(self._lib.icpmi_staged_merged_points(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 4), dtype=np.float32)
        if n.value:
            self._check(self._lib.icpmi_staged_merged_points(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def stagedBinCells(self, cell_size=20.0, capacity=4096):
        """icpmi_staged_bin_cells: the last epoch's merged set binned on the device and appended to the handle's cell log;
        returns (ijk [c, 3] int32, offsets [c] int64, counts [c] int64), cells in the order of their first point."""
        ijk = np.empty((int(capacity), 3), dtype=np.int32)
        off = np.empty(int(capacity), dtype=np.int64)
        cnt = np.empty(int(capacity), dtype=np.int64)
        nc = C.c_int64(0)
        self._check(self._lib.icpmi_staged_bin_cells(self._h, cell_size, ijk.ctypes.data, off.ctypes.data, cnt.ctypes.data, int(capacity), C.byref(nc)))
        return ijk[:nc.value].copy(), off[:nc.value].copy(), cnt[:nc.value].copy()

    def cellLogConfigure(self, cell_size):
        """icpmi_cell_log_configure: cell_size > 0 -- every epoch enqueues the binning of its merged set itself; stagedBinCells(cell_size) collects it."""
        self._check(self._lib.icpmi_cell_log_configure(self._h, float(cell_size)))

    def cellLogSize(self):
        n = C.c_int64(0)
        self._check(self._lib.icpmi_cell_log_read(self._h, 0, 0, None, C.byref(n)))
        return int(n.value)

    def cellLogRead(self, offset, count):
        """icpmi_cell_log_read: `count` points of the device-resident cell log from `offset`."""
        out = np.empty((int(count), 4), dtype=np.float32)
        if count:
            self._check(self._lib.icpmi_cell_log_read(self._h, int(offset), int(count), out.ctypes.data, None))
        return out

    def cellLogClear(self):
        self._check(self._lib.icpmi_cell_log_clear(self._h))

    def stageDiscard(self):
        """icpmi_stage_discard: drop the scan staged by registerWithPrior."""
        self._check(self._lib.icpmi_stage_discard(self._h))
        self._staged_n = 0

    def getMap(self, with_normals=False):
        """The resident map in the caller's order (Map::getLocalPointCloud, Map.cpp:536-540)."""
        m = C.c_int64(0)
        self._check(self._lib.icpmi_get_map(self._h, None, None, 0, C.byref(m)))
        out = np.empty((m.value, 4), dtype=np.float32)
        nrm = np.empty((m.value, 3), dtype=np.float32) if with_normals else None
        if m.value:
            self._check(self._lib.icpmi_get_map(self._h, out.ctypes.data, None if nrm is None else nrm.ctypes.data, m.value, C.byref(m)))
        return (out, nrm) if with_normals else out

    def binCells(self, cloud, cell_size=20.0):
        c = _f32c(cloud, 4)
        out = np.empty((c.shape[0], 3), dtype=np.int32)
        self._check(self._lib.icpmi_bin_cells(self._h, c.ctypes.data, c.shape[0], cell_size, out.ctypes.data))
        return out

    def setStream(self, hip_stream_ptr):
        self._check(self._lib.icpmi_set_stream(self._h, hip_stream_ptr))

    def lastMatches(self, n=None):
        """icpmi_debug_last_matches: (ids (n, k) int32, d2 (n, k) float32, T_used 4x4) of the last counted iteration of the last single
        registration, rows in the reading's order; T_used is the centred-frame pose its queries were moved by.  n defaults to the size of
        the last reading registered through this object."""
        n = self._last_n if n is None else int(n)
        k = int(self.cfg.knn)
        ids = np.empty((n, k), dtype=np.int32)
        d2 = np.empty((n, k), dtype=np.float32)
        T = (C.c_float * 16)()
        self._check(self._lib.icpmi_debug_last_matches(self._h, n, k, ids.ctypes.data, d2.ctypes.data, T))
        return ids, d2, _T_from_c(T[:])

    def debugSelfKnn(self, cloud, k, with_info=False):
        """icpmi_debug_self_knn: (ids (m, k) int32 original indices, d2 (m, k) float32) of the self k-NN search behind surfaceNormals, on the same
        private search handle; with_info: also a dict of the grid that call built (cell, na, tsize, queued, trials)."""
        c = _f32c(cloud, 4); m = c.shape[0]; k = int(k)
        ids = np.empty((m, k), dtype=np.int32); d2 = np.empty((m, k), dtype=np.float32)
        info = (C.c_uint64 * 8)()
        self._check(self._lib.icpmi_debug_self_knn(self._h, c.ctypes.data, m, k, ids.ctypes.data, d2.ctypes.data, info if with_info else None))
        if not with_info:
            return ids, d2
        cell = float(np.array([info[0]], dtype=np.uint32).view(np.float32)[0])
        return ids, d2, {"cell": cell, "na": (int(info[1]), int(info[2]), int(info[3])), "tsize": int(info[4]), "queued": int(info[5]),
                         "trials": int(info[6])}

    def debugMergeBlocks(self, blocks, min_dist, stride=None, mode=0, capacity=None):
        """icpmi_debug_merge_blocks: the epoch's rank-ordered merge on `blocks` (one (n_r, 4) array per rank, empty ones included), block r
        laid at r * stride (default: the largest count).  mode 0: the epoch's choice of kernel, 1: the per-block launches.  Returns
        (merged (n, 4) float32, [kept (n_r,) bool per block], path); capacity (default: all) bounds the copy-out only -- merged then holds
        what fits and the full count is returned as a fourth value."""
        blocks = [_f32c(b, 4) for b in blocks]
        counts = np.array([b.shape[0] for b in blocks], dtype=np.int64)
        total = int(counts.sum())
        if stride is None:
            stride = int(counts.max()) if counts.size else 0
        pts = np.concatenate(blocks) if total else np.zeros((0, 4), dtype=np.float32)
        cap = total if capacity is None else int(capacity)
        out = np.empty((max(cap, 1), 4), dtype=np.float32)
        kept = np.zeros(max(total, 1), dtype=np.uint8)
        mn, path = C.c_int64(0), C.c_int32(-1)
        self._check(self._lib.icpmi_debug_merge_blocks(self._h, pts.ctypes.data if total else None, counts.ctypes.data if counts.size else None,
                                                       len(blocks), int(stride), float(min_dist), int(mode), out.ctypes.data, cap, C.byref(mn),
                                                       kept.ctypes.data, C.byref(path)))
        ends = np.cumsum(counts)
        kept_list = [kept[e - n:e].astype(bool) for e, n in zip(ends, counts)]
        merged = out[:min(mn.value, cap)].copy()
        if capacity is None:
            return merged, kept_list, int(path.value)
        return merged, kept_list, int(path.value), int(mn.value)

    def debugResidentKthD2(self):
        """icpmi_debug_resident_kth_d2: (d2 of every resident point's k-th neighbour (m,) float32, that k) as the last append-only update's
        SurfaceNormal pass remembered them; raises when they do not describe the resident map."""
        m = C.c_int64(0)
        self._check(self._lib.icpmi_get_map(self._h, None, None, 0, C.byref(m)))
        out = np.empty(max(m.value, 1), dtype=np.float32)
        knn = C.c_int32(0)
        self._check(self._lib.icpmi_debug_resident_kth_d2(self._h, m.value, out.ctypes.data, C.byref(knn)))
        return out[:m.value], int(knn.value)

    def debugIndexNormals(self):
        """icpmi_debug_index_normals: (sorted (m, 3) float32, pn (m, 3) float32 or None) -- the normals the registration index holds, rows by
        original index as getMap's: the sorted copy, and the copy interleaved with the points where the handle keeps one."""
        m = C.c_int64(0)
        self._check(self._lib.icpmi_get_map(self._h, None, None, 0, C.byref(m)))
        srt = np.full((max(m.value, 1), 3), np.nan, dtype=np.float32)
        pn = np.full((max(m.value, 1), 3), np.nan, dtype=np.float32)
        has = C.c_int32(0)
        self._check(self._lib.icpmi_debug_index_normals(self._h, m.value, srt.ctypes.data, pn.ctypes.data, C.byref(has)))
        return srt[:m.value], (pn[:m.value] if has.value else None)

    def keepSums(self, on=1):
        """icpmi_debug_keep_sums: from now on (on) / no longer (off) keep the pair sums of this handle's single registrations for lastSums();
        off by default.  Drops the cached loop graphs."""
        self._check(self._lib.icpmi_debug_keep_sums(self._h, 1 if on else 0))

    def lastSums(self):
        """icpmi_debug_last_sums: (sums (32,) float64 in icpmi_minimize_step's layout, limits (8,) float32, robust_scale, vt_ratio) of the last
        counted iteration of the last single registration; needs keepSums(1) before that registration."""
        sums = (C.c_double * 32)()
        lim = (C.c_float * 8)()
        rs, vt = C.c_float(), C.c_float()
        self._check(self._lib.icpmi_debug_last_sums(self._h, sums, lim, C.byref(rs), C.byref(vt)))
        return np.array(sums[:], dtype=np.float64), np.array(lim[:], dtype=np.float32), np.float32(rs.value), np.float32(vt.value)

    def debugCounters(self):
        """icpmi_debug_counters: 24 diagnostic words of the last registration (include/icpmi.h; 10 / 11: queries the k = 1 matcher's helper
        workgroups ran / far-seeded queries that found the defer list full)."""
        out = (C.c_uint64 * 24)()
        self._check(self._lib.icpmi_debug_counters(self._h, out))
        return list(out)

    def gridInfo(self):
        cell = C.c_float()
        dims = (C.c_int32 * 3)()
        nc, no = C.c_int64(), C.c_int64()
        self._check(self._lib.icpmi_get_grid_info(self._h, C.byref(cell), dims, C.byref(nc), C.byref(no)))
        return {"cell": cell.value, "dims": list(dims), "n_cells": nc.value, "n_occupied": no.value}
