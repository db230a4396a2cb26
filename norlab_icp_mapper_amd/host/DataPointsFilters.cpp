// DataPointsFilters.cpp -- the DataPointsFilter classes, their factory and the chain (declarations: IcpSequence.h;
// semantics: SURVEY.md B.9).
#include "IcpSequence.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <random>

namespace nim {

namespace {
// std::minstd_rand (x <- 48271 x mod 2^31 - 1: fully specified by the C++ standard, so the oracle restates it) and the two ways
// upstream turns it into [0, 1): randomSamplingMethod 0 "direct" = x / float(max - min), 1 "uniform" =
// std::uniform_real_distribution<float> = (x - min) / float(max - min + 1) capped below 1 (libstdc++'s generate_canonical).
struct MinStd {
    uint32_t x;
    explicit MinStd(uint32_t seed) : x(seed % 2147483647u) { if (x == 0) x = 1; }
    uint32_t next() { x = (uint32_t)(((uint64_t)x * 48271ull) % 2147483647ull); return x; }
    float unit(int method) {
        const uint32_t v = next();
        if (method == 1) { const float r = (float)(v - 1u) / 2147483646.0f; return r < 1.0f ? r : std::nextafter(1.0f, 0.0f); }
        return (float)v / 2147483645.0f; // max() - min() = 2147483646 - 1
    }
};

struct DistanceLimitFilter : DataPointsFilter {
    int dim = -1; float dist = 1.f; bool removeInside = true;
    bool pointFilter(icpmi_point_filter& f) const override {
        f = icpmi_point_filter{}; f.type = ICPMI_FILT_DISTANCE_LIMIT; f.i = dim; f.f[0] = dist; f.f[1] = removeInside ? 1.f : 0.f;
        return dim >= -1 && dim <= 2;
    }
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        std::vector<uint8_t> keep(n);
        const float ad = std::fabs(dist);
        for (size_t i = 0; i < n; ++i) {
            const float* p = c.col(i);
            const float v = dim < 0 ? std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) : std::fabs(p[dim]);
            keep[i] = removeInside ? v > ad : v < ad;
        }
        c.keepOnly(keep);
    }
};

struct BoundingBoxFilter : DataPointsFilter {
    float lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1}; bool removeInside = true;
    bool pointFilter(icpmi_point_filter& f) const override {
        f = icpmi_point_filter{}; f.type = ICPMI_FILT_BOUNDING_BOX; f.i = removeInside ? 1 : 0;
        for (int r = 0; r < 3; ++r) { f.f[r] = lo[r]; f.f[3 + r] = hi[r]; }
        return true;
    }
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        std::vector<uint8_t> keep(n);
        for (size_t i = 0; i < n; ++i) {
            const float* p = c.col(i);
            bool inside = true;
            for (int r = 0; r < 3; ++r) inside &= p[r] > lo[r] && p[r] < hi[r];
            keep[i] = removeInside ? !inside : inside;
        }
        c.keepOnly(keep);
    }
};

struct AddDescriptorFilter : DataPointsFilter {
    std::string name; int dimension = 1; std::vector<float> values;
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        std::vector<float> data((size_t)dimension * n);
        for (size_t i = 0; i < n; ++i) for (int r = 0; r < dimension; ++r) data[(size_t)dimension * i + r] = values[r];
        c.addDescriptor(name, dimension, std::move(data));
    }
};

struct CutAtDescriptorThresholdFilter : DataPointsFilter {
    std::string name; bool useLargerThan = true; float threshold = 0.f;
    bool residentOp(icpmi_map_op& op, std::string& scalarName) const override {
        op = icpmi_map_op{}; op.type = ICPMI_MOP_CUT_SCALAR; op.i = useLargerThan ? 1 : 0; op.f[0] = threshold;
        scalarName = name;
        return true;
    }
    void inPlaceFilter(DataPoints& c) const override {
        const Descriptor& d = c.getDescriptorByName(name);
        const size_t n = c.getNbPoints();
        std::vector<uint8_t> keep(n);
        for (size_t i = 0; i < n; ++i) {
            const float v = d.data[(size_t)d.span * i];
            keep[i] = useLargerThan ? !(v > threshold) : !(v < threshold);
        }
        c.keepOnly(keep);
    }
};

struct SurfaceNormalFilter : DataPointsFilter {
    icpmi_handle h; int knn = 5; bool keepDensities = false, keepMatchedIds = false, keepMeanDist = false, keepEigenValues = false, keepEigenVectors = false;
    int surfaceNormalKnn() const override { return knn; }
    bool residentOp(icpmi_map_op& op, std::string&) const override {
        op = icpmi_map_op{}; op.type = ICPMI_MOP_SURFACE_NORMALS; op.i = knn; op.f[0] = keepDensities ? 1.f : 0.f;
        // the resident map tracks `densities` (the same pass writes the row); not `matchedIds`, `meanDist` or the eigen rows
        return knn >= 1 && knn <= 32 && !keepMatchedIds && !keepMeanDist && !keepEigenValues && !keepEigenVectors;
    }
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        std::vector<float> normals(3 * n), dens(keepDensities ? n : 0), md(keepMeanDist ? n : 0);
        std::vector<int32_t> ids(keepMatchedIds ? n * (size_t)knn : 0);
        std::vector<float> eva(keepEigenValues ? 3 * n : 0), eve(keepEigenVectors ? 9 * n : 0);
        GpuICPSequence::check(h, icpmi_surface_normals_ex3(h, c.features.data(), (int64_t)n, knn, normals.data(), keepDensities ? dens.data() : nullptr,
                                                           keepMatchedIds ? ids.data() : nullptr, keepMeanDist ? md.data() : nullptr,
                                                           keepEigenValues ? eva.data() : nullptr, keepEigenVectors ? eve.data() : nullptr));
        c.addDescriptor("normals", 3, std::move(normals));
        if (keepEigenValues) c.addDescriptor("eigValues", 3, std::move(eva));     // (upstream's descriptor names)
        if (keepEigenVectors) c.addDescriptor("eigVectors", 9, std::move(eve));
        if (keepDensities) c.addDescriptor("densities", 1, std::move(dens));
        if (keepMatchedIds) { // upstream stores the ids as descriptor rows of the cloud's scalar type
            std::vector<float> f(ids.size());
            for (size_t i = 0; i < ids.size(); ++i) f[i] = (float)ids[i];
            c.addDescriptor("matchedIds", knn, std::move(f));
        }
        if (keepMeanDist) c.addDescriptor("meanDist", 1, std::move(md));
    }
};

// RandomSamplingDataPointsFilter{prob 0.75, randomSamplingMethod 0, seed -1} [UPSTREAM 1.4.x, as recalled]: a fresh
// std::minstd_rand per call (seed -1: std::random_device), one number per point, point kept iff number < prob, never more
// than floor(n * prob) + 1 points.
struct RandomSamplingFilter : DataPointsFilter {
    float prob = 0.75f; int method = 0; int seed = -1;
    bool repeatable() const override { return seed != -1; }
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        const size_t nOut = (size_t)((float)n * prob);
        MinStd rng(seed == -1 ? (uint32_t)std::random_device()() : (uint32_t)seed);
        std::vector<uint8_t> keep(n, 0);
        size_t j = 0;
        for (size_t i = 0; i < n && j <= nOut; ++i)
            if (rng.unit(method) < prob) { keep[i] = 1; ++j; }
        c.keepOnly(keep);
    }
};

// MaxDensityDataPointsFilter{maxDensity 10} [UPSTREAM]: needs `densities` (SurfaceNormalDataPointsFilter{keepDensities: 1});
// a point in a region denser than maxDensity survives with probability maxDensity / density.
struct MaxDensityFilter : DataPointsFilter {
    float maxDensity = 10.f; int seed = 1;
    // the resident step draws from the `densities` row a SurfaceNormal{keepDensities: 1} step of the same program wrote (Map::residentPlan
    // checks that one stands in front); a maxDensity the device entry refuses stays with the host loop
    bool residentOp(icpmi_map_op& op, std::string&) const override {
        op = icpmi_map_op{}; op.type = ICPMI_MOP_MAX_DENSITY; op.f[0] = maxDensity; op.i = seed;
        return std::isfinite(maxDensity) && maxDensity > 0.f;
    }
    void inPlaceFilter(DataPoints& c) const override {
        if (!c.descriptorExists("densities")) throw InvalidField("MaxDensityDataPointsFilter: Error, no densities found in descriptors.");
        const Descriptor& d = c.getDescriptorByName("densities");
        const size_t n = c.getNbPoints();
        MinStd rng((uint32_t)seed);
        std::vector<uint8_t> keep(n, 1);
        for (size_t i = 0; i < n; ++i) {
            const float density = d.data[(size_t)d.span * i];
            if (density > maxDensity) keep[i] = rng.unit(0) < maxDensity / density;
        }
        c.keepOnly(keep);
    }
};

struct IdentityFilter : DataPointsFilter { void inPlaceFilter(DataPoints&) const override {} };

// A run of sensor-model filters (ObservationDirection / OrientNormals / Shadow / SimpleSensorNoise; include/icpmi.h:
// icpmi_sensor_model) as one device pass.  The missing-descriptor errors are raised here, in chain order, with the texts of the
// filters; afterwards the container is touched exactly as filtering one by one touches it: every ObservationDirection /
// OrientNormals step moves its descriptor to the end, SimpleSensorNoise adds or replaces its row, and one keepOnly compacts the
// points and every row -- those produced after the Shadow step included -- when the run holds a Shadow step.
void applySensorRun(icpmi_handle h, DataPoints& cl, const icpmi_sensor_step* steps, size_t count)
{
    const size_t n = cl.getNbPoints();
    bool haveOd = false, needsNormals = false, needsOdIn = false, orient = false, shadow = false, noise = false;
    for (size_t k = 0; k < count; ++k) {
        switch (steps[k].type) {
            case ICPMI_SM_OBSERVATION_DIRECTION: haveOd = true; break;
            case ICPMI_SM_ORIENT_NORMALS:
                if (!cl.descriptorExists("normals")) throw InvalidField("OrientNormalsDataPointsFilter: Error, cannot find normals in descriptors.");
                if (!haveOd && !cl.descriptorExists("observationDirections")) throw InvalidField("OrientNormalsDataPointsFilter: Error, cannot find observation directions in descriptors.");
                if (cl.getDescriptorByName("normals").span != 3 || (!haveOd && cl.getDescriptorByName("observationDirections").span != 3))
                    throw InvalidField("OrientNormalsDataPointsFilter: normals and observationDirections must have 3 rows");
                needsNormals = orient = true; needsOdIn |= !haveOd;
                break;
            case ICPMI_SM_SHADOW:
                if (!cl.descriptorExists("normals")) throw InvalidField("ShadowDataPointsFilter: Error, cannot find normals in descriptors");
                if (cl.getDescriptorByName("normals").span != 3) throw InvalidField("ShadowDataPointsFilter: normals must have 3 rows");
                needsNormals = shadow = true;
                break;
            default: noise = true; break;
        }
    }
    std::vector<float> nrm(orient ? 3 * n : 0), od(haveOd ? 3 * n : 0), nz(noise ? n : 0);
    std::vector<uint8_t> keep(shadow ? n : 0);
    GpuICPSequence::check(h, icpmi_sensor_model(h, cl.features.data(), (int64_t)n, needsNormals ? cl.getDescriptorByName("normals").data.data() : nullptr,
                                                needsOdIn ? cl.getDescriptorByName("observationDirections").data.data() : nullptr, steps, (int32_t)count,
                                                orient ? nrm.data() : nullptr, haveOd ? od.data() : nullptr, noise ? nz.data() : nullptr,
                                                shadow ? keep.data() : nullptr));
    for (size_t k = 0; k < count; ++k) {
        if (steps[k].type == ICPMI_SM_OBSERVATION_DIRECTION) { cl.removeDescriptor("observationDirections"); cl.addDescriptor("observationDirections", 3, od); }
        else if (steps[k].type == ICPMI_SM_ORIENT_NORMALS) { cl.removeDescriptor("normals"); cl.addDescriptor("normals", 3, nrm); }
        else if (steps[k].type == ICPMI_SM_SIMPLE_SENSOR_NOISE) cl.addDescriptor("simpleSensorNoise", 1, nz);
    }
    if (shadow) cl.keepOnly(keep);
}

// ObservationDirectionDataPointsFilter{x 0, y 0, z 0} [UPSTREAM]: descriptor `observationDirections` = sensor position - point
// (3 rows; it rotates with the cloud like `normals`, RigidTransformation::compute).  inPlaceFilter is the path of a chain without a
// GPU context; with one, DataPointsFilters::apply runs the step on the device (applySensorRun), with the same bits.
struct ObservationDirectionFilter : DataPointsFilter {
    float c[3] = {0, 0, 0};
    bool sensorStep(icpmi_sensor_step& s) const override {
        s = icpmi_sensor_step{}; s.type = ICPMI_SM_OBSERVATION_DIRECTION; for (int r = 0; r < 3; ++r) s.f[r] = c[r];
        return true;
    }
    void inPlaceFilter(DataPoints& cl) const override {
        const size_t n = cl.getNbPoints();
        std::vector<float> d(3 * n);
        for (size_t i = 0; i < n; ++i) { const float* p = cl.col(i); for (int r = 0; r < 3; ++r) d[3 * i + r] = c[r] - p[r]; }
        if (cl.descriptorExists("observationDirections")) cl.removeDescriptor("observationDirections");
        cl.addDescriptor("observationDirections", 3, std::move(d));
    }
};

// OrientNormalsDataPointsFilter{towardCenter 1} [UPSTREAM]: a normal whose scalar product with the observation direction is
// negative (towardCenter) / positive (away) is flipped; needs `normals` and `observationDirections`.  inPlaceFilter: as above.
struct OrientNormalsFilter : DataPointsFilter {
    bool towardCenter = true;
    bool sensorStep(icpmi_sensor_step& s) const override {
        s = icpmi_sensor_step{}; s.type = ICPMI_SM_ORIENT_NORMALS; s.i = towardCenter ? 1 : 0;
        return true;
    }
    void inPlaceFilter(DataPoints& cl) const override {
        if (!cl.descriptorExists("normals")) throw InvalidField("OrientNormalsDataPointsFilter: Error, cannot find normals in descriptors.");
        if (!cl.descriptorExists("observationDirections")) throw InvalidField("OrientNormalsDataPointsFilter: Error, cannot find observation directions in descriptors.");
        Descriptor nrm = cl.getDescriptorByName("normals");
        const Descriptor& od = cl.getDescriptorByName("observationDirections");
        if (nrm.span != 3 || od.span != 3) throw InvalidField("OrientNormalsDataPointsFilter: normals and observationDirections must have 3 rows");
        const size_t n = cl.getNbPoints();
        for (size_t i = 0; i < n; ++i) {
            const float dot = nrm.data[3 * i] * od.data[3 * i] + nrm.data[3 * i + 1] * od.data[3 * i + 1] + nrm.data[3 * i + 2] * od.data[3 * i + 2];
            if (towardCenter ? dot < 0.f : dot > 0.f) for (int r = 0; r < 3; ++r) nrm.data[3 * i + r] = -nrm.data[3 * i + r];
        }
        cl.removeDescriptor("normals");
        cl.addDescriptor("normals", 3, std::move(nrm.data));
    }
};

// ShadowDataPointsFilter{eps 0.1} (libpointmatcher, as recalled; the formulation is icpmi_sensor_model's in include/icpmi.h): drops
// the points whose normal is nearly perpendicular to the beam, | n / |n| . p / |p| | <= eps -- the sensor is the cloud's origin.
// Device only; a run of one when it stands alone.
struct ShadowFilter : DataPointsFilter {
    float eps = 0.1f;
    icpmi_handle h = nullptr;
    bool sensorStep(icpmi_sensor_step& s) const override {
        s = icpmi_sensor_step{}; s.type = ICPMI_SM_SHADOW; s.f[0] = eps;
        return true;
    }
    void inPlaceFilter(DataPoints& cl) const override {
        if (!h) throw std::logic_error("ShadowDataPointsFilter needs a GPU context");
        icpmi_sensor_step s; sensorStep(s);
        applySensorRun(h, cl, &s, 1);
    }
};

// SimpleSensorNoiseDataPointsFilter{sensorType 0, gain 1} (libpointmatcher, as recalled; icpmi_sensor_model): descriptor
// `simpleSensorNoise` (1 row), the range noise of the sensor model at the point's distance from the origin -- what
// ErrorMinimizer::getOverlap() reads (GpuICPSequence::operator()).  Device only; a run of one when it stands alone.
struct SimpleSensorNoiseFilter : DataPointsFilter {
    int sensorType = 0; float gain = 1.f;
    icpmi_handle h = nullptr;
    bool sensorStep(icpmi_sensor_step& s) const override {
        s = icpmi_sensor_step{}; s.type = ICPMI_SM_SIMPLE_SENSOR_NOISE; s.i = sensorType; s.f[0] = gain;
        return true;
    }
    void inPlaceFilter(DataPoints& cl) const override {
        if (!h) throw std::logic_error("SimpleSensorNoiseDataPointsFilter needs a GPU context");
        icpmi_sensor_step s; sensorStep(s);
        applySensorRun(h, cl, &s, 1);
    }
};

struct RemoveNaNFilter : DataPointsFilter {
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        std::vector<uint8_t> keep(n);
        for (size_t i = 0; i < n; ++i) { const float* p = c.col(i); keep[i] = !(std::isnan(p[0]) || std::isnan(p[1]) || std::isnan(p[2])); }
        c.keepOnly(keep);
    }
};

// symmetric 3x3 eigen-decomposition (cyclic Jacobi, double): eigenvalues w, eigenvectors in the columns of Q
static void jacobi3(const double C[9], double w[3], double Q[9])
{
    double A[3][3] = {{C[0], C[3], C[6]}, {C[1], C[4], C[7]}, {C[2], C[5], C[8]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 60; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double dg = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off <= 1e-32 * dg || off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 3; ++k) { const double a = A[k][p], b = A[k][q]; A[k][p] = cs * a - sn * b; A[k][q] = sn * a + cs * b; }
                for (int k = 0; k < 3; ++k) { const double a = A[p][k], b = A[q][k]; A[p][k] = cs * a - sn * b; A[q][k] = sn * a + cs * b; }
                for (int k = 0; k < 3; ++k) { const double a = V[k][p], b = V[k][q]; V[k][p] = cs * a - sn * b; V[k][q] = sn * a + cs * b; }
            }
    }
    for (int e = 0; e < 3; ++e) { w[e] = A[e][e]; for (int r = 0; r < 3; ++r) Q[3 * e + r] = V[r][e]; }
}

// SamplingSurfaceNormalDataPointsFilter{ratio 0.5, knn 7, samplingMethod 0, maxBoxDim inf, averageExistingDescriptors 1,
// keepNormals 1} [UPSTREAM, as recalled] -- the reference filter of PM::ICPSequence::setDefault (Mapper.cpp:77): the cloud is
// split at the median of its widest dimension until a box holds at most knn points; every box gets ONE normal (smallest
// eigenvector of the covariance of its points; boxes of rank < 2 or wider than maxBoxDim are dropped), and its points are kept
// with probability `ratio` (samplingMethod 0) or replaced by their mean (1).  Output in box order.  Deterministic here: the
// median split orders by (coordinate, index), points inside a box by index, the random numbers are MinStd(seed) (upstream:
// std::nth_element's permutation and std::rand).  Host code: a recursive median split is what the reference runs on the CPU
// too; it runs once per setMap.
struct SamplingSurfaceNormalFilter : DataPointsFilter {
    icpmi_handle h = nullptr; // GPU context (createDataPointsFilter): the device path of inPlaceFilter
    float ratio = 0.5f; int knn = 7; int method = 0; float maxBoxDim = INFINITY; bool averageDescriptors = true; bool keepNormals = true; int seed = 1;
    struct Work {
        const DataPoints* in; DataPoints out; std::vector<float> normals; MinStd rng; const SamplingSurfaceNormalFilter* f;
        Work(const DataPoints* c, const SamplingSurfaceNormalFilter* ff) : in(c), out(c->createSimilarEmpty()), rng((uint32_t)ff->seed), f(ff) {}
    };
    // column j of `out` gets, in every descriptor row, the mean over the `cnt` members `mem` of `in` (ascending index order, summed in double)
    static void meanDescriptors(const DataPoints& in, const int32_t* mem, size_t cnt, DataPoints& out, size_t j) {
        for (size_t d = 0; d < in.descriptors.size(); ++d) {
            const Descriptor& src = in.descriptors[d];
            for (int r = 0; r < src.span; ++r) {
                double s2 = 0;
                for (size_t k = 0; k < cnt; ++k) s2 += src.data[(size_t)src.span * mem[k] + r];
                out.descriptors[d].data[(size_t)src.span * j + r] = (float)(s2 / (double)cnt);
            }
        }
    }
    void fuse(Work& w, std::vector<int32_t>& idx, size_t first, size_t last) const {
        const size_t cnt = last - first;
        std::sort(idx.begin() + first, idx.begin() + last);
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double mean[3] = {0, 0, 0};
        for (size_t k = first; k < last; ++k) {
            const float* p = w.in->col((size_t)idx[k]);
            for (int r = 0; r < 3; ++r) { lo[r] = std::min(lo[r], p[r]); hi[r] = std::max(hi[r], p[r]); mean[r] += p[r]; }
        }
        if (std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2])) > maxBoxDim) return;
        for (int r = 0; r < 3; ++r) mean[r] /= (double)cnt;
        double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t k = first; k < last; ++k) {
            const float* p = w.in->col((size_t)idx[k]);
            const double v[3] = {p[0] - mean[0], p[1] - mean[1], p[2] - mean[2]};
            for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) C[3 * c + r] += v[r] * v[c];
        }
        double ev[3], Q[9];
        jacobi3(C, ev, Q);
        const double wmax = std::max(std::fabs(ev[0]), std::max(std::fabs(ev[1]), std::fabs(ev[2])));
        int rank = 0;
        for (int e = 0; e < 3; ++e) if (wmax > 0 && std::fabs(ev[e]) > 3.0 * 1.1920928955078125e-07 * wmax) ++rank;
        if (rank < 2) return; // the points of the box are "unfit"
        int e = 0;
        if (ev[1] < ev[e]) e = 1;
        if (ev[2] < ev[e]) e = 2;
        const float nrm[3] = {(float)Q[3 * e], (float)Q[3 * e + 1], (float)Q[3 * e + 2]};
        if (method == 1) {
            w.out.appendColFrom(*w.in, (size_t)idx[first]);
            const size_t j = w.out.getNbPoints() - 1;
            for (int r = 0; r < 3; ++r) w.out.col(j)[r] = (float)mean[r];
            if (averageDescriptors) meanDescriptors(*w.in, idx.data() + first, cnt, w.out, j);
            w.normals.insert(w.normals.end(), nrm, nrm + 3);
            return;
        }
        for (size_t k = first; k < last; ++k)
            if (w.rng.unit(0) < ratio) { w.out.appendColFrom(*w.in, (size_t)idx[k]); w.normals.insert(w.normals.end(), nrm, nrm + 3); }
    }
    void build(Work& w, std::vector<int32_t>& idx, size_t first, size_t last, const float lo[3], const float hi[3]) const {
        const size_t cnt = last - first;
        if (cnt == 0) return;
        if (cnt <= (size_t)knn) { fuse(w, idx, first, last); return; }
        int dim = 0;
        for (int r = 1; r < 3; ++r) if (hi[r] - lo[r] > hi[dim] - lo[dim]) dim = r;
        const size_t right = cnt / 2, left = cnt - right;
        const DataPoints* in = w.in;
        auto less = [in, dim](int32_t a, int32_t b) { const float x = in->col((size_t)a)[dim], y = in->col((size_t)b)[dim]; return x < y || (x == y && a < b); };
        std::nth_element(idx.begin() + first, idx.begin() + first + left, idx.begin() + last, less);
        const float cut = in->col((size_t)idx[first + left])[dim];
        float lhi[3] = {hi[0], hi[1], hi[2]}, rlo[3] = {lo[0], lo[1], lo[2]};
        lhi[dim] = cut; rlo[dim] = cut;
        build(w, idx, first, first + left, lo, lhi);
        build(w, idx, first + left, last, rlo, hi);
    }
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        if (n == 0) return;
        if (h && method == 0 && knn >= 3 && seed >= 0) {
            // r3: the partition, the box normals and the sampling run on the device (csrc/ssn.hip: one radix sort per tree level) -- the
            // filter sits on the REFERENCE of the default chain, i.e. on the whole map at every icp.setMap; the host recursion below
            // (one thread) is what a shell WITHOUT a GPU context runs (the CPU-only unit tests of the host classes)
            std::vector<int32_t> order(n);
            std::vector<float> nrm(3 * n);
            int64_t kept = 0;
            GpuICPSequence::check(h, icpmi_sampling_surface_normal(h, c.features.data(), (int64_t)n, ratio, knn, maxBoxDim, seed, order.data(), nrm.data(), &kept));
            DataPoints out = c.select(order.data(), (size_t)kept);
            nrm.resize(3 * (size_t)kept);
            if (keepNormals) out.addDescriptor("normals", 3, std::move(nrm));
            c = std::move(out);
            return;
        }
        if (h && method == 1 && knn >= 3) {
            // r5: samplingMethod 1 on the device too -- partition, box normals and box means by csrc/ssn.hip; what stays here is the
            // bookkeeping of the container: the kept column per box and, with averageExistingDescriptors, the mean of every descriptor
            // row over the members the device lists (descriptor rows live in this container, not on the device)
            std::vector<int32_t> order(n), ms(n), mc(n), mem(n);
            std::vector<float> nrm(3 * n), mean(3 * n);
            int64_t boxes = 0;
            GpuICPSequence::check(h, icpmi_sampling_surface_normal_ex(h, c.features.data(), (int64_t)n, 1.0f, knn, maxBoxDim, seed < 0 ? 1 : seed, 1, order.data(),
                                                                      nrm.data(), &boxes, mean.data(), ms.data(), mc.data(), mem.data()));
            DataPoints out = c.select(order.data(), (size_t)boxes);
            for (size_t b = 0; b < (size_t)boxes; ++b) {
                for (int r = 0; r < 3; ++r) out.col(b)[r] = mean[3 * b + r];
                if (averageDescriptors) meanDescriptors(c, mem.data() + ms[b], (size_t)mc[b], out, b);
            }
            nrm.resize(3 * (size_t)boxes);
            if (keepNormals) out.addDescriptor("normals", 3, std::move(nrm));
            c = std::move(out);
            return;
        }
        std::vector<int32_t> idx(n);
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t i = 0; i < n; ++i) { idx[i] = (int32_t)i; for (int r = 0; r < 3; ++r) { lo[r] = std::min(lo[r], c.col(i)[r]); hi[r] = std::max(hi[r], c.col(i)[r]); } }
        Work w(&c, this);
        build(w, idx, 0, n, lo, hi);
        if (keepNormals) w.out.addDescriptor("normals", 3, std::move(w.normals));
        c = std::move(w.out);
    }
};

// OctreeGridDataPointsFilter (created at OctreeMapperModule.cpp:12, applied at :38): octree over the bounding
// cube of the cloud, split until the node edge is <= maxSizeByNode or the node holds <= maxPointByNode points, one point per
// leaf, the cloud left in leaf-visiting order.  The tree lives on the device (icpmi_octree_sample / ICPMI_MOP_OCTREE):
// samplingMethod 0 (first point of the leaf) and 1 (random point, made reproducible) pick there; 2 (centroid: features and
// descriptors averaged over the leaf) and 3 (medoid: the point with the smallest summed distance to the others of its leaf)
// are formed here from the device's leaf assignment.  `times` are those of the column the filter kept: the selected point
// (0, 1, 3), or for the centroid the leaf's representative, whose slot receives the averages (as VoxelGrid: the first point's values).
struct OctreeGridFilter : DataPointsFilter {
    float maxSize = 0.f; int method = 0; int maxPointByNode = 1;
    icpmi_handle h = nullptr;
    bool residentOp(icpmi_map_op& op, std::string&) const override {
        op = icpmi_map_op{}; op.type = ICPMI_MOP_OCTREE; op.i = method; op.f[0] = maxSize; op.f[1] = (float)maxPointByNode;
        return (method == 0 || method == 1) && maxSize >= 0.f && maxPointByNode <= 64;
    }
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        if (n == 0) return;
        if (!h) throw std::logic_error("OctreeGridDataPointsFilter needs a GPU context");
        std::vector<int32_t> order(n), leaf;
        if (method >= 2) leaf.resize(n);
        int64_t m = 0;
        GpuICPSequence::check(h, icpmi_octree_sample(h, c.features.data(), (int64_t)n, maxSize, maxPointByNode, method == 1 ? 1 : 0, order.data(),
                                                     method >= 2 ? leaf.data() : nullptr, &m));
        order.resize((size_t)m);
        if (method <= 1) { c = c.select(order.data(), order.size()); return; }
        // members of every leaf, in list order
        std::vector<std::vector<int32_t>> members((size_t)m);
        for (size_t i = 0; i < n; ++i) members[(size_t)leaf[i]].push_back((int32_t)i);
        if (method == 3) { // medoid
            for (size_t l = 0; l < (size_t)m; ++l) {
                const auto& mem = members[l];
                double best = INFINITY; int32_t pick = mem[0];
                for (int32_t a : mem) {
                    double sum = 0;
                    for (int32_t b : mem) {
                        double d2 = 0;
                        for (int r = 0; r < 3; ++r) { const double e = (double)c.col((size_t)a)[r] - c.col((size_t)b)[r]; d2 += e * e; }
                        sum += std::sqrt(d2);
                    }
                    if (sum < best) { best = sum; pick = a; }
                }
                order[l] = pick;
            }
            c = c.select(order.data(), order.size());
            return;
        }
        DataPoints out = c.select(order.data(), order.size()); // centroid: the representative's slot receives the leaf's averages
        for (size_t l = 0; l < (size_t)m; ++l) {
            const auto& mem = members[l];
            const double inv = 1.0 / (double)mem.size();
            for (int r = 0; r < 3; ++r) { double s2 = 0; for (int32_t i : mem) s2 += c.col((size_t)i)[r]; out.col(l)[r] = (float)(s2 * inv); }
            for (size_t k = 0; k < c.descriptors.size(); ++k) {
                const Descriptor& d = c.descriptors[k];
                for (int r = 0; r < d.span; ++r) { double s2 = 0; for (int32_t i : mem) s2 += d.data[(size_t)d.span * i + r]; out.descriptors[k].data[(size_t)d.span * l + r] = (float)(s2 * inv); }
            }
        }
        c = std::move(out);
    }
};

// VoxelGridDataPointsFilter{vSizeX, vSizeY, vSizeZ, useCentroid, averageExistingDescriptors} (libpointmatcher, as recalled;
// the formulation is icpmi_voxel_grid's in include/icpmi.h): one point per occupied voxel of upstream's bounding-box lattice, the
// centroid of its members, in ascending order of the voxel's first point.  The grid, the sort and the sums live on the device; here
// every descriptor row is packed point-major for it, and the cloud is rebuilt with the names, spans and order of the input.  `times`
// keep the first point's values.  useCentroid: 0 is refused at creation.
struct VoxelGridFilter : DataPointsFilter {
    float vsize[3] = {1.f, 1.f, 1.f}; bool averageDescriptors = true;
    icpmi_handle h = nullptr;
    bool movesFeatures() const override { return true; }
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        if (n == 0) return;
        if (!h) throw std::logic_error("VoxelGridDataPointsFilter needs a GPU context");
        int rows = 0;
        for (const auto& d : c.descriptors) rows += d.span;
        std::vector<float> desc((size_t)rows * n), descOut((size_t)rows * n), out4(4 * n);
        for (size_t i = 0, r0 = 0; i < c.descriptors.size(); r0 += (size_t)c.descriptors[i].span, ++i) {
            const Descriptor& d = c.descriptors[i];
            for (size_t p = 0; p < n; ++p)
                for (int r = 0; r < d.span; ++r) desc[(size_t)rows * p + r0 + r] = d.data[(size_t)d.span * p + r];
        }
        std::vector<int32_t> order(n);
        int64_t m = 0;
        GpuICPSequence::check(h, icpmi_voxel_grid(h, c.features.data(), (int64_t)n, vsize, averageDescriptors ? 1 : 0, rows ? desc.data() : nullptr, rows,
                                                  order.data(), out4.data(), rows ? descOut.data() : nullptr, &m));
        DataPoints out = c.select(order.data(), (size_t)m); // every voxel's first point: its `times` stay, the device's values replace the rest
        out.features.assign(out4.begin(), out4.begin() + 4 * m);
        for (size_t i = 0, r0 = 0; i < out.descriptors.size(); r0 += (size_t)out.descriptors[i].span, ++i) {
            Descriptor& d = out.descriptors[i];
            for (size_t p = 0; p < (size_t)m; ++p)
                for (int r = 0; r < d.span; ++r) d.data[(size_t)d.span * p + r] = descOut[(size_t)rows * p + r0 + r];
        }
        c = std::move(out);
    }
};

// CovarianceSamplingDataPointsFilter{nbSample, torqueNorm} (libpointmatcher, Gelfand et al. 2003, as recalled; the formulation is
// icpmi_covariance_sampling's in include/icpmi.h): keeps nbSample points chosen greedily to constrain the six pose directions evenly,
// in selection order.  The whole selection runs on the device; here features, every descriptor and `times` follow the order.
struct CovarianceSamplingFilter : DataPointsFilter {
    int64_t nbSample = 5000; int torqueNorm = 1;
    icpmi_handle h = nullptr;
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        if ((size_t)nbSample >= n) return;
        const Descriptor& nrm = c.getDescriptorByName("normals"); // (InvalidField without normals, as upstream)
        if (nrm.span != 3) throw InvalidField("descriptor normals must have 3 rows");
        if (!h) throw std::logic_error("CovarianceSamplingDataPointsFilter needs a GPU context");
        std::vector<int32_t> order((size_t)nbSample);
        int64_t m = 0;
        GpuICPSequence::check(h, icpmi_covariance_sampling(h, c.features.data(), (int64_t)n, nrm.data.data(), nbSample, torqueNorm, order.data(), &m,
                                                           nullptr));
        c = c.select(order.data(), (size_t)m);
    }
};

// NormalSpaceDataPointsFilter{nbSample, seed, epsilon} (libpointmatcher, Rusinkiewicz & Levoy 2001, as recalled; the formulation is
// icpmi_normal_space_sampling's in include/icpmi.h): keeps nbSample points spread evenly over the angular buckets of the normals, in
// ascending index order.  The draw within a bucket follows std::minstd_rand(seed), never a random device: always repeatable().  The
// whole selection runs on the device; here features, every descriptor and `times` follow the kept indices.
struct NormalSpaceFilter : DataPointsFilter {
    int64_t nbSample = 5000; int seed = 1; float epsilon = 0.09817f;
    icpmi_handle h = nullptr;
    void inPlaceFilter(DataPoints& c) const override {
        const size_t n = c.getNbPoints();
        if ((size_t)nbSample >= n) return;
        const Descriptor& nrm = c.getDescriptorByName("normals"); // (InvalidField without normals, as upstream)
        if (nrm.span != 3) throw InvalidField("descriptor normals must have 3 rows");
        if (!h) throw std::logic_error("NormalSpaceDataPointsFilter needs a GPU context");
        std::vector<int32_t> order((size_t)nbSample);
        int64_t m = 0;
        GpuICPSequence::check(h, icpmi_normal_space_sampling(h, c.features.data(), (int64_t)n, nrm.data.data(), nbSample, seed, epsilon, order.data(), &m,
                                                             nullptr));
        c = c.select(order.data(), (size_t)m);
    }
};

float getf(const yaml::Node& p, const char* k, float def) { return p[k] ? p[k].as<float>() : def; }
int geti(const yaml::Node& p, const char* k, int def) { return p[k] ? p[k].as<int>() : def; }

} // namespace

// test seam (TestHooks.cpp: nim_test_minstd_nth): the raw n-th value of the host filters' generator
uint32_t minstdNth(uint32_t seed, uint32_t n) { MinStd g(seed); uint32_t v = g.x; for (uint32_t i = 0; i < n; ++i) v = g.next(); return v; }

std::shared_ptr<DataPointsFilter> createDataPointsFilter(const std::string& name, const yaml::Node& p, icpmi_handle ctx)
{
    if (name == "DistanceLimitDataPointsFilter") {
        requireKnown(p, {"dim", "dist", "removeInside"}, name);
        auto f = std::make_shared<DistanceLimitFilter>();
        f->dim = geti(p, "dim", -1); f->dist = getf(p, "dist", 1.f); f->removeInside = geti(p, "removeInside", 1) != 0;
        if (f->dim > 2) throw InvalidParameter(name + ": dim out of range");
        return f;
    }
    if (name == "BoundingBoxDataPointsFilter") {
        requireKnown(p, {"xMin", "xMax", "yMin", "yMax", "zMin", "zMax", "removeInside"}, name);
        auto f = std::make_shared<BoundingBoxFilter>();
        f->lo[0] = getf(p, "xMin", -1); f->hi[0] = getf(p, "xMax", 1);
        f->lo[1] = getf(p, "yMin", -1); f->hi[1] = getf(p, "yMax", 1);
        f->lo[2] = getf(p, "zMin", -1); f->hi[2] = getf(p, "zMax", 1);
        f->removeInside = geti(p, "removeInside", 1) != 0;
        return f;
    }
    if (name == "AddDescriptorDataPointsFilter") {
        requireKnown(p, {"descriptorName", "descriptorDimension", "descriptorValues"}, name);
        auto f = std::make_shared<AddDescriptorFilter>();
        if (!p["descriptorName"]) throw InvalidParameter(name + ": descriptorName is required");
        f->name = p["descriptorName"].as<std::string>();
        f->dimension = geti(p, "descriptorDimension", 1);
        if (p["descriptorValues"].IsSequence()) for (const auto& v : p["descriptorValues"].seq) f->values.push_back(v.as<float>());
        else if (p["descriptorValues"].IsScalar()) f->values.push_back(p["descriptorValues"].as<float>());
        if ((int)f->values.size() != f->dimension) throw InvalidParameter(name + ": descriptorValues must have descriptorDimension entries");
        return f;
    }
    if (name == "CutAtDescriptorThresholdDataPointsFilter") {
        requireKnown(p, {"descName", "useLargerThan", "threshold"}, name);
        auto f = std::make_shared<CutAtDescriptorThresholdFilter>();
        f->name = p["descName"] ? p["descName"].as<std::string>() : "none";
        f->useLargerThan = geti(p, "useLargerThan", 1) != 0; f->threshold = getf(p, "threshold", 0.f);
        return f;
    }
    if (name == "SurfaceNormalDataPointsFilter") {
        requireKnown(p, {"knn", "maxDist", "epsilon", "keepNormals", "keepDensities", "keepEigenValues", "keepEigenVectors",
                         "keepMatchedIds", "keepMeanDist", "sortEigen", "smoothNormals"}, name);
        if (geti(p, "smoothNormals", 0) != 0) throw InvalidParameter(name + ": smoothNormals is not on the accelerated path");
        // r5: keepEigenValues / keepEigenVectors are served in ASCENDING eigenvalue order, i.e. together with sortEigen: 1; upstream's unsorted
        // order is whatever Eigen::EigenSolver returns for the matrix at hand and is not reproduced
        if ((geti(p, "keepEigenValues", 0) != 0 || geti(p, "keepEigenVectors", 0) != 0) && geti(p, "sortEigen", 0) == 0)
            throw InvalidParameter(name + ": keepEigenValues / keepEigenVectors are served with sortEigen: 1 only (the unsorted order is the eigen-solver's)");
        auto f = std::make_shared<SurfaceNormalFilter>();
        f->h = ctx; f->knn = geti(p, "knn", 5); f->keepDensities = geti(p, "keepDensities", 0) != 0;
        f->keepEigenValues = geti(p, "keepEigenValues", 0) != 0; f->keepEigenVectors = geti(p, "keepEigenVectors", 0) != 0;
        f->keepMatchedIds = geti(p, "keepMatchedIds", 0) != 0; f->keepMeanDist = geti(p, "keepMeanDist", 0) != 0;
        return f;
    }
    if (name == "RandomSamplingDataPointsFilter") {
        requireKnown(p, {"prob", "randomSamplingMethod", "seed"}, name);
        auto f = std::make_shared<RandomSamplingFilter>();
        f->prob = getf(p, "prob", 0.75f); f->method = geti(p, "randomSamplingMethod", 0); f->seed = geti(p, "seed", -1);
        if (!(f->prob >= 0.f && f->prob <= 1.f) || f->method < 0 || f->method > 1 || f->seed < -1) throw InvalidParameter(name + ": parameter out of range");
        return f;
    }
    if (name == "SamplingSurfaceNormalDataPointsFilter") {
        requireKnown(p, {"ratio", "knn", "samplingMethod", "maxBoxDim", "averageExistingDescriptors", "keepNormals", "keepDensities", "keepEigenValues",
                         "keepEigenVectors", "seed"}, name);
        for (const char* k : {"keepDensities", "keepEigenValues", "keepEigenVectors"})
            if (geti(p, k, 0) != 0) throw InvalidParameter(name + ": " + k + " is not supported");
        auto f = std::make_shared<SamplingSurfaceNormalFilter>();
        f->h = ctx;
        f->ratio = getf(p, "ratio", 0.5f); f->knn = geti(p, "knn", 7); f->method = geti(p, "samplingMethod", 0);
        f->maxBoxDim = p["maxBoxDim"] ? p["maxBoxDim"].as<float>() : INFINITY;
        f->averageDescriptors = geti(p, "averageExistingDescriptors", 1) != 0; f->keepNormals = geti(p, "keepNormals", 1) != 0;
        f->seed = geti(p, "seed", 1);
        if (!(f->ratio > 0.f && f->ratio <= 1.f) || f->knn < 3 || f->method < 0 || f->method > 1) throw InvalidParameter(name + ": parameter out of range");
        return f;
    }
    if (name == "MaxDensityDataPointsFilter") {
        requireKnown(p, {"maxDensity", "seed"}, name);
        auto f = std::make_shared<MaxDensityFilter>();
        f->maxDensity = getf(p, "maxDensity", 10.f); f->seed = geti(p, "seed", 1);
        if (!(f->maxDensity > 0.f)) throw InvalidParameter(name + ": maxDensity must be > 0");
        return f;
    }
    if (name == "IdentityDataPointsFilter") return std::make_shared<IdentityFilter>();
    if (name == "ObservationDirectionDataPointsFilter") {
        requireKnown(p, {"x", "y", "z"}, name);
        auto f = std::make_shared<ObservationDirectionFilter>();
        f->c[0] = getf(p, "x", 0.f); f->c[1] = getf(p, "y", 0.f); f->c[2] = getf(p, "z", 0.f);
        return f;
    }
    if (name == "OrientNormalsDataPointsFilter") {
        requireKnown(p, {"towardCenter"}, name);
        auto f = std::make_shared<OrientNormalsFilter>();
        f->towardCenter = geti(p, "towardCenter", 1) != 0;
        return f;
    }
    if (name == "ShadowDataPointsFilter") {
        requireKnown(p, {"eps"}, name);
        auto f = std::make_shared<ShadowFilter>();
        f->eps = getf(p, "eps", 0.1f);
        if (!(f->eps >= 0.f && f->eps <= 1.f)) throw InvalidParameter(name + ": eps must be in [0, 1]");
        f->h = ctx;
        return f;
    }
    if (name == "SimpleSensorNoiseDataPointsFilter") {
        requireKnown(p, {"sensorType", "gain"}, name);
        auto f = std::make_shared<SimpleSensorNoiseFilter>();
        f->sensorType = geti(p, "sensorType", 0); f->gain = getf(p, "gain", 1.f);
        if (f->sensorType < 0 || f->sensorType > 4)
            throw InvalidParameter(name + ": sensorType must be 0 (Sick LMS-1xx), 1 (Hokuyo URG-04LX), 2 (Hokuyo UTM-30LX), 3 (Kinect) or 4 (Xtion)");
        if (!(f->gain > 0.f) || !std::isfinite(f->gain)) throw InvalidParameter(name + ": gain must be finite and > 0");
        f->h = ctx;
        return f;
    }
    if (name == "MinDistDataPointsFilter" || name == "MaxDistDataPointsFilter") {
        // the older names of DistanceLimitDataPointsFilter: MinDist{dim -1, minDist 1} keeps what lies beyond, MaxDist{dim -1, maxDist 1} within
        const bool isMin = name == "MinDistDataPointsFilter";
        requireKnown(p, {"dim", isMin ? "minDist" : "maxDist"}, name);
        auto f = std::make_shared<DistanceLimitFilter>();
        f->dim = geti(p, "dim", -1); f->dist = getf(p, isMin ? "minDist" : "maxDist", 1.f); f->removeInside = isMin;
        if (f->dim < -1 || f->dim > 2) throw InvalidParameter(name + ": dim must be in [-1, 2]");
        return f;
    }
    if (name == "RemoveNaNDataPointsFilter") return std::make_shared<RemoveNaNFilter>();
    if (name == "OctreeGridDataPointsFilter") {
        requireKnown(p, {"buildParallel", "maxPointByNode", "maxSizeByNode", "samplingMethod"}, name);
        auto f = std::make_shared<OctreeGridFilter>();
        f->maxSize = getf(p, "maxSizeByNode", 0.f); f->method = geti(p, "samplingMethod", 0);
        f->maxPointByNode = geti(p, "maxPointByNode", 1);
        if (f->maxSize < 0.f || f->maxPointByNode < 1 || f->method < 0 || f->method > 3) throw InvalidParameter(name + ": parameter out of range");
        f->h = ctx;
        return f;
    }
    if (name == "VoxelGridDataPointsFilter") {
        requireKnown(p, {"vSizeX", "vSizeY", "vSizeZ", "useCentroid", "averageExistingDescriptors"}, name);
        if (geti(p, "useCentroid", 1) == 0)
            throw InvalidParameter(name + ": useCentroid: 0 (voxel centres) is not supported: upstream's centre branch, as recalled, "
                                          "writes the centre without the grid origin and cannot be checked");
        auto f = std::make_shared<VoxelGridFilter>();
        f->vsize[0] = getf(p, "vSizeX", 1.f); f->vsize[1] = getf(p, "vSizeY", 1.f); f->vsize[2] = getf(p, "vSizeZ", 1.f);
        for (float v : f->vsize)
            if (!(v > 0.f) || !std::isfinite(v)) throw InvalidParameter(name + ": vSizeX / vSizeY / vSizeZ must be finite and > 0");
        f->averageDescriptors = geti(p, "averageExistingDescriptors", 1) != 0;
        f->h = ctx;
        return f;
    }
    if (name == "CovarianceSamplingDataPointsFilter") {
        requireKnown(p, {"nbSample", "torqueNorm"}, name);
        auto f = std::make_shared<CovarianceSamplingFilter>();
        f->nbSample = geti(p, "nbSample", 5000);
        f->torqueNorm = geti(p, "torqueNorm", 1);
        if (f->nbSample < 0) throw InvalidParameter(name + ": nbSample must be >= 0");
        if (f->torqueNorm < 0 || f->torqueNorm > 2) throw InvalidParameter(name + ": torqueNorm must be 0 (L1), 1 (Lavg) or 2 (Lmax)");
        f->h = ctx;
        return f;
    }
    if (name == "NormalSpaceDataPointsFilter") {
        requireKnown(p, {"nbSample", "seed", "epsilon"}, name);
        auto f = std::make_shared<NormalSpaceFilter>();
        // (64-bit: a seed above 2147483647 is refused, not wrapped)
        auto getll = [&](const char* k, long long def) {
            if (!p[k]) return def;
            const std::string s = p[k].str();
            char* end = nullptr;
            const long long v = std::strtoll(s.c_str(), &end, 10);
            if (end == s.c_str() || *end) throw yaml::Exception("bad integer: " + s);
            return v;
        };
        const long long nb = getll("nbSample", 5000), seed = getll("seed", 1);
        f->epsilon = getf(p, "epsilon", 0.09817f);
        if (nb < 1) throw InvalidParameter(name + ": nbSample must be >= 1");
        if (seed < 0 || seed > 2147483647ll) throw InvalidParameter(name + ": seed must be in [0, 2147483647]");
        if (!(f->epsilon >= 0.04908f && f->epsilon <= 3.14159f)) throw InvalidParameter(name + ": epsilon must be in [0.04908, 3.14159]");
        f->nbSample = nb; f->seed = (int)seed;
        f->h = ctx;
        return f;
    }
    throw InvalidParameter("unknown DataPointsFilter " + name);
}

void DataPointsFilters::apply(DataPoints& cloud, const DataPointsFilter* leading) const
{
    static const bool fuse = [] { const char* e = std::getenv("NIM_FUSED_INPUT_FILTERS"); return !e || std::atoi(e) != 0; }();
    std::vector<const DataPointsFilter*> chain;
    if (leading) chain.push_back(leading);
    for (const auto& f : filters) chain.push_back(f.get());
    size_t i = 0;
    while (i < chain.size()) {
        std::vector<icpmi_sensor_step> steps;
        icpmi_sensor_step st;
        while (fuse && ctx && i + steps.size() < chain.size() && steps.size() < 8 && chain[i + steps.size()]->sensorStep(st)) steps.push_back(st);
        if (!steps.empty()) { // (a run of one takes the same path)
            applySensorRun(ctx, cloud, steps.data(), steps.size());
            i += steps.size();
            continue;
        }
        std::vector<icpmi_point_filter> run;
        icpmi_point_filter pf;
        while (fuse && ctx && i + run.size() < chain.size() && run.size() < 16 && chain[i + run.size()]->pointFilter(pf)) run.push_back(pf);
        if (run.size() >= 2 && cloud.getNbPoints() > 0) {
            std::vector<uint8_t> keep(cloud.getNbPoints());
            GpuICPSequence::check(ctx, icpmi_filter_points(ctx, cloud.features.data(), (int64_t)cloud.getNbPoints(), run.data(), (int32_t)run.size(), keep.data()));
            cloud.keepOnly(keep);
            i += run.size();
        } else {
            chain[i]->inPlaceFilter(cloud);
            ++i;
        }
    }
}

DataPointsFilters::DataPointsFilters(const yaml::Node& seq, icpmi_handle ctx_) : ctx(ctx_)
{
    icpmi_handle ctx = ctx_;
    if (!seq) return;
    if (!seq.IsSequence()) throw yaml::Exception("expected a sequence of filters");
    for (const auto& item : seq.seq) {
        auto e = singleEntry(item, "DataPointsFilter");
        filters.push_back(createDataPointsFilter(e.first, e.second, ctx));
    }
}

} // namespace nim
