// api.hip -- the extern "C" surface declared in include/icpmi.h (see that header for the reference
// interface each entry point replaces).
#include "common.h"
#include <cstring>
#include <new>
#include <dlfcn.h>
#include <mutex>
#include <cstdio>

static std::string g_create_error;

// ICPMI_ROCTX=1: every entry point that takes a handle runs inside a roctx range named after it (rocprofv3 --marker-trace
// then shows registrations, map updates and merges as ranges above their kernels).  The marker library is looked up at run
// time: nothing links against it, and without the variable the cost is one predictable branch per call.
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        const char* e = getenv("ICPMI_ROCTX");
        if (!e || !atoi(e)) return;
        // rocprofv3 --marker-trace follows the SDK's marker library; the roctracer one is the fall-back for older tools
        for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1",
                                 "libroctx64.so.4", "libroctx64.so", "/opt/rocm/lib/libroctx64.so.4"}) {
            void* lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (!lib) continue;
            push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
            pop = (int (*)())dlsym(lib, "roctxRangePop");
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
Roctx& roctx() { static Roctx r; return r; }
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
    ~RoctxRange() { if (on) roctx().pop(); }
};
} // namespace

// locks the handle for the rest of the calling function (see icpmi_ctx::mu) and makes its device current
#define CHECK_H(h)                                                           \
    RoctxRange _roctx_range(__func__);                                       \
    if (!(h)) return ICPMI_ERR_INVALID_ARG;                                  \
    std::lock_guard<std::recursive_mutex> _handle_lock((h)->mu);             \
    do {                                                                     \
        hipError_t _e = hipSetDevice((h)->device);                           \
        if (_e != hipSuccess) {                                              \
            (h)->last_error = std::string("hipSetDevice: ") + hipGetErrorString(_e); \
            return ICPMI_ERR_HIP;                                            \
        }                                                                    \
        if ((h)->zero_pending && zero_state_if_pending(h) != ICPMI_OK) return ICPMI_ERR_HIP; \
    } while (0)

extern "C" {

int32_t icpmi_version(void) { return ICPMI_VERSION; }
#ifndef ICPMI_SRC_STAMP
#define ICPMI_SRC_STAMP "unstamped"
#endif
#define ICPMI_STR2(x) #x
#define ICPMI_STR(x) ICPMI_STR2(x)
const char* icpmi_build_info(void) { return "icpmi " ICPMI_STR(ICPMI_VERSION) " src:" ICPMI_SRC_STAMP; }

void icpmi_config_default(icpmi_config* cfg)
{
    memset(cfg, 0, sizeof *cfg);
    cfg->device = 0;
    cfg->knn = 1;
    cfg->max_dist = INFINITY;
    cfg->epsilon = 0.f;
    cfg->n_outlier = 0;
    cfg->minimizer = ICPMI_MIN_POINT_TO_PLANE;
    cfg->max_iterations = 40;
    cfg->use_differential = 0;
    cfg->min_diff_rot = 0.001f;
    cfg->min_diff_trans = 0.001f;
    cfg->smooth_length = 3;
    cfg->use_bound = 0;
    cfg->max_rot_norm = 1.f;
    cfg->max_trans_norm = 1.f;
    cfg->grid_cell = 0.f;
    cfg->use_graph = 1;
    cfg->profile = 0;
    cfg->covariance = 0;
    cfg->sensor_std_dev = 0.01f; // PointToPlaneWithCovErrorMinimizer.sensorStdDev
}

static icpmi_status validate_config(const icpmi_config* cfg, std::string& err)
{
    if (cfg->knn < 1 || cfg->knn > ICPMI_MAX_K) { err = "InvalidParameter: knn must be in [1, 32]"; return ICPMI_ERR_INVALID_ARG; }
    if (cfg->var_dist != 0 && cfg->var_dist != 1) { err = "InvalidParameter: var_dist must be 0 or 1"; return ICPMI_ERR_INVALID_ARG; }
    if (!cfg->var_dist && !(cfg->max_dist > 0.f)) { err = "InvalidParameter: maxDist must be > 0"; return ICPMI_ERR_INVALID_ARG; } // (KDTreeVarDistMatcher has no maxDist)
    if (cfg->epsilon < 0.f) { err = "InvalidParameter: epsilon must be >= 0"; return ICPMI_ERR_INVALID_ARG; }
    if (cfg->n_outlier < 0 || cfg->n_outlier > ICPMI_MAX_OUTLIER) { err = "InvalidParameter: at most 8 outlier filters"; return ICPMI_ERR_INVALID_ARG; }
    for (int f = 0; f < cfg->n_outlier; ++f) {
        const int t = cfg->outlier[f].type;
        const float p = cfg->outlier[f].param;
        if (t < ICPMI_OUT_MAXDIST || t > ICPMI_OUT_VARTRIMMEDDIST) { err = "InvalidParameter: unknown outlier filter type"; return ICPMI_ERR_INVALID_ARG; }
        if (t == ICPMI_OUT_VARTRIMMEDDIST) {
            const float lo = cfg->outlier[f].param, hi = cfg->outlier[f].param2, lam = cfg->outlier[f].param3;
            if (!(lo > 0.f && lo < 1.f) || !(hi > 0.f && hi < 1.f) || !(lo <= hi) || !(lam >= 0.f)) { // upstream: ratios in ]0, 1[, lambda >= 0
                err = "InvalidParameter: VarTrimmedDist needs 0 < minRatio <= maxRatio < 1 and lambda >= 0"; return ICPMI_ERR_INVALID_ARG;
            }
        }
        if (t == ICPMI_OUT_GENERICDESCRIPTOR) {
            const int ip = cfg->outlier[f].iparam;
            if (ip & ~7) { err = "InvalidParameter: GenericDescriptorOutlierFilter: unknown flag"; return ICPMI_ERR_INVALID_ARG; }
        }
        if (t == ICPMI_OUT_ROBUST) {
            const int ip = cfg->outlier[f].iparam;
            if ((ip & 15) > ICPMI_ROB_STUDENT || ((ip >> 4) & 15) > ICPMI_SCALE_STD || ((ip >> 8) & 15) > ICPMI_DIST_POINT2PLANE || (ip >> 12)) {
                err = "InvalidParameter: RobustOutlierFilter: unknown robustFct / scaleEstimator / distanceType"; return ICPMI_ERR_INVALID_ARG;
            }
            if (!(cfg->outlier[f].param2 >= 0.f)) { err = "InvalidParameter: RobustOutlierFilter: nbIterationForScale must be >= 0"; return ICPMI_ERR_INVALID_ARG; }
            if (!(cfg->outlier[f].param3 >= 0.f)) { err = "InvalidParameter: RobustOutlierFilter: approximation must be >= 0 (0 or +inf: none)"; return ICPMI_ERR_INVALID_ARG; }
        }
        if (t == ICPMI_OUT_TRIMMEDDIST && !(p >= 0.f && p <= 1.f)) { err = "InvalidParameter: TrimmedDist ratio must be in [0, 1]"; return ICPMI_ERR_INVALID_ARG; }
        if ((t == ICPMI_OUT_MAXDIST || t == ICPMI_OUT_MINDIST || t == ICPMI_OUT_MEDIANDIST) && !(p >= 0.f)) { err = "InvalidParameter: negative outlier filter parameter"; return ICPMI_ERR_INVALID_ARG; }
    }
    if (cfg->minimizer < ICPMI_MIN_IDENTITY || cfg->minimizer > ICPMI_MIN_PLANE_TO_PLANE) { err = "InvalidParameter: unknown error minimizer"; return ICPMI_ERR_INVALID_ARG; }
    if (cfg->minimizer == ICPMI_MIN_PLANE_TO_PLANE) {
        if (cfg->force_2d || cfg->is_2d) { err = "InvalidParameter: PlaneToPlaneErrorMinimizer: no planar mode (force2D / 2-D clouds)"; return ICPMI_ERR_INVALID_ARG; }
        if (cfg->covariance) { err = "InvalidParameter: PlaneToPlaneErrorMinimizer: no pose covariance (Censi's form is derived for the scalar point-to-plane residual)"; return ICPMI_ERR_INVALID_ARG; }
        if (cfg->degeneracy_threshold != 0.f) { err = "InvalidParameter: PlaneToPlaneErrorMinimizer: no degeneracyThreshold (mu = lambda / sum w assumes unit-information pairs)"; return ICPMI_ERR_INVALID_ARG; }
    }
    if (cfg->force_4dof && cfg->force_2d) { err = "InvalidParameter: force2D and force4DOF exclude each other"; return ICPMI_ERR_INVALID_ARG; }
    if (cfg->max_iterations < 1) { err = "InvalidParameter: maxIterationCount must be >= 1"; return ICPMI_ERR_INVALID_ARG; }
    if (cfg->use_differential && (cfg->smooth_length < 1 || cfg->smooth_length > ICPMI_MAX_SMOOTH)) { err = "InvalidParameter: smoothLength must be in [1, 16]"; return ICPMI_ERR_INVALID_ARG; }
    if (cfg->grid_cell < 0.f) { err = "InvalidParameter: grid_cell must be >= 0"; return ICPMI_ERR_INVALID_ARG; }
    if (cfg->covariance != 0 && cfg->covariance != 1) { err = "InvalidParameter: covariance must be 0 or 1"; return ICPMI_ERR_INVALID_ARG; }
    if (cfg->covariance) {
        if (cfg->minimizer != ICPMI_MIN_POINT_TO_PLANE) { err = "InvalidParameter: PointToPlaneWithCovErrorMinimizer: the covariance needs the point-to-plane minimizer"; return ICPMI_ERR_INVALID_ARG; }
        if (cfg->is_2d) { err = "InvalidParameter: PointToPlaneWithCovErrorMinimizer: no covariance of planar (2-D) clouds"; return ICPMI_ERR_INVALID_ARG; }
        if (!std::isfinite(cfg->sensor_std_dev) || cfg->sensor_std_dev < 0.f) { err = "InvalidParameter: PointToPlaneWithCovErrorMinimizer: sensorStdDev must be finite and >= 0"; return ICPMI_ERR_INVALID_ARG; }
    }
    if (cfg->degeneracy_threshold != 0.f) {
        if (!std::isfinite(cfg->degeneracy_threshold)) { err = "InvalidParameter: degeneracyThreshold must be finite"; return ICPMI_ERR_INVALID_ARG; }
        if (cfg->minimizer != ICPMI_MIN_POINT_TO_PLANE) { err = "InvalidParameter: degeneracyThreshold needs the point-to-plane minimizer"; return ICPMI_ERR_INVALID_ARG; }
        if (cfg->force_2d || cfg->is_2d) { err = "InvalidParameter: degeneracyThreshold: no degeneracy analysis with force2D or of planar (2-D) clouds"; return ICPMI_ERR_INVALID_ARG; }
    }
    return ICPMI_OK;
}

// KDTreeVarDistMatcher ignores max_dist: the handle keeps +inf, so that the index is built with every pyramid level -- the row, and with it the
// bound of a search, arrives with each reading
static void store_config(icpmi_ctx* c, const icpmi_config* cfg)
{
    c->cfg = *cfg;
    if (c->cfg.var_dist) c->cfg.max_dist = INFINITY;
}

} // extern "C"

// a handle without the allocation cache's handle count: what icpmi_create wraps, and what the private handles of the map-side operators are made of
icpmi_status create_handle(const icpmi_config* cfg, icpmi_handle* out)
{
    if (!cfg || !out) { g_create_error = "icpmi_create: null argument"; return ICPMI_ERR_INVALID_ARG; }
    *out = nullptr;
    icpmi_status vs = validate_config(cfg, g_create_error);
    if (vs != ICPMI_OK) return vs;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("icpmi_create: no HIP device available (") + hipGetErrorString(e) + ")";
        return ICPMI_ERR_HIP;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "icpmi_create: device ordinal out of range"; return ICPMI_ERR_INVALID_ARG; }
    icpmi_ctx* c = new (std::nothrow) icpmi_ctx();
    if (!c) { g_create_error = "icpmi_create: out of host memory"; return ICPMI_ERR_HIP; }
    store_config(c, cfg);
    c->device = cfg->device;
    { // the k = 1 matcher's helper workgroups (nn.hip: nn1_wg_kernel), as the environment stands now: ICPMI_NN_DEFER=0 keeps every query at
      // home, ICPMI_NN_DEFER_WGS = how many helpers a launch gets (rounded up to a multiple of 8; eight list entries each)
        const char* e = getenv("ICPMI_NN_DEFER");
        c->nn_defer = !(e && *e && atoi(e) == 0);
        const char* w = getenv("ICPMI_NN_DEFER_WGS");
        int wgs = (w && *w) ? atoi(w) : ICPMI_NN_DEFER_WGS_DEFAULT;
        wgs = (wgs + 7) / 8 * 8;
        if (wgs <= 0) c->nn_defer = false;
        c->nn_defer_wgs = wgs < 8 ? 8 : (wgs > ICPMI_NN_DEFER_WGS_MAX ? ICPMI_NN_DEFER_WGS_MAX : wgs);
    }
#define CR(expr)                                                                                      \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            g_create_error = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
            icpmi_destroy(c);                                                                         \
            return ICPMI_ERR_HIP;                                                                     \
        }                                                                                             \
    } while (0)
    CR(hipSetDevice(c->device));
    CR(stream_acquire(&c->stream));
    c->own_stream = true;
    CR(c->d_state.alloc(ICPMI_MAX_BATCH));
    c->zero_pending = true; // (common.h: zero_state_if_pending -- neither the legacy stream, which breaks another thread's capture, nor a stream this handle may never use)
    CR(c->d_selhist.alloc(ICPMI_SELHIST_WORDS));
    CR(hipHostMalloc((void**)&c->h_state, sizeof(IcpState) * ICPMI_MAX_BATCH, hipHostMallocMapped));
    memset(c->h_state, 0, sizeof(IcpState) * ICPMI_MAX_BATCH);
    if (hipHostGetDevicePointer((void**)&c->d_state_mirror, c->h_state, 0) != hipSuccess) { c->d_state_mirror = nullptr; (void)hipGetLastError(); } // (then loop_run copies)
    CR(hipHostMalloc((void**)&c->h_pin, ICPMI_PIN_BYTES + ICPMI_UP_SLOT * ICPMI_UP_SLOTS, hipHostMallocDefault));
    CR(hipHostMalloc((void**)&c->h_nocc, 64, hipHostMallocDefault));
    *c->h_nocc = 0;
    if (hipHostGetDevicePointer((void**)&c->d_nocc_host, c->h_nocc, 0) != hipSuccess) c->d_nocc_host = nullptr; // (then the copy launch stays)
    CR(hipHostMalloc((void**)&c->h_progress, ICPMI_PROGRESS_WORDS * sizeof(unsigned), hipHostMallocMapped)); // words 0..15: progress per reading of a batch; word 32: sequence number of the registration being launched
    memset(c->h_progress, 0, ICPMI_PROGRESS_WORDS * sizeof(unsigned));
    CR(hipHostGetDevicePointer((void**)&c->d_progress, c->h_progress, 0));
    CR(hipEventCreate(&c->ev0));
    CR(hipEventCreate(&c->ev1));
#undef CR
    *out = c;
    return ICPMI_OK;
}

extern "C" {

// handles the CALLER creates count towards the allocation cache's lifetime (private handles are created through create_handle directly)
icpmi_status icpmi_create(const icpmi_config* cfg, icpmi_handle* out)
{
    const icpmi_status s = create_handle(cfg, out);
    if (s == ICPMI_OK) {
        (*out)->counted = true;
        DevBlockCache& bc = dev_block_cache();
        std::lock_guard<std::mutex> lk(bc.mu);
        ++bc.handles;
    }
    return s;
}

icpmi_status icpmi_set_config(icpmi_handle h, const icpmi_config* cfg)
{
    CHECK_H(h);
    if (!cfg) { h->last_error = "set_config: null config"; return ICPMI_ERR_INVALID_ARG; }
    icpmi_status vs = validate_config(cfg, h->last_error);
    if (vs != ICPMI_OK) return vs;
    if (cfg->device != h->device) { h->last_error = "set_config: the device of a handle cannot change"; return ICPMI_ERR_INVALID_ARG; }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    store_config(h, cfg);
    h->degen_ready = false; // (a report belongs to the chain that produced it)
    // the cached loop graph was captured for the previous chain
    drop_loop_graphs(h);
    return ICPMI_OK;
}

void icpmi_destroy(icpmi_handle c)
{
    if (!c) return;
    if (c->temp) { icpmi_destroy(c->temp); c->temp = nullptr; }
    if (c->temp_raw) { icpmi_destroy(c->temp_raw); c->temp_raw = nullptr; }
    hipSetDevice(c->device);
    selfgrid_destroy(c);
    comm_destroy(c);
    if (c->stream) hipStreamSynchronize(c->stream);
    c->graphs.reset();
    // ONE device-wide wait for all of the handle's blocks, which free themselves when the handle is deleted below (common.h: DevFreeSynced)
    DevFreeSynced synced;
    if (c->h_state) hipHostFree(c->h_state);
    if (c->h_pin) hipHostFree(c->h_pin);
    if (c->h_nocc) hipHostFree(c->h_nocc);
    if (c->h_progress) hipHostFree(c->h_progress);
    if (c->h_cells) (void)hipHostFree(c->h_cells);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->nn_events) hipEventDestroy(e);
    if (c->side_fork) hipEventDestroy(c->side_fork);
    if (c->side_join) hipEventDestroy(c->side_join);
    if (c->side) stream_release(c->side);
    if (c->own_stream && c->stream) stream_release(c->stream);
    const bool counted = c->counted;
    delete c;
    if (counted) { // (bookkeeping only: a mapper that is dropped and rebuilt -- the replay harness, one per pass -- finds its blocks again;
                   //  a host that wants the memory back calls icpmi_trim_cache(), measured r6: trimming here cost every new mapper ~300 hipMalloc)
        DevBlockCache& bc = dev_block_cache();
        std::lock_guard<std::mutex> lk(bc.mu);
        if (--bc.handles < 0) bc.handles = 0;
    }
}

// every device block the library's allocation cache holds back to the runtime (common.h: DevBlockCache); handles stay valid
icpmi_status icpmi_trim_cache(void)
{
    dev_cache_trim();
    return ICPMI_OK;
}


const char* icpmi_last_error(icpmi_handle h) { return h ? h->last_error.c_str() : g_create_error.c_str(); }

icpmi_status icpmi_set_stream(icpmi_handle h, void* hip_stream)
{
    CHECK_H(h);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->own_stream && h->stream) stream_release(h->stream);
    h->stream = (hipStream_t)hip_stream;
    h->own_stream = false;
    drop_loop_graphs(h);
    return ICPMI_OK;
}

int32_t icpmi_has_map(icpmi_handle h) { return h && h->m > 0 ? 1 : 0; }

icpmi_status icpmi_get_map_mean(icpmi_handle h, float mean3[3])
{
    if (!h || !mean3) return ICPMI_ERR_INVALID_ARG;
    memcpy(mean3, h->mean, 3 * sizeof(float));
    return ICPMI_OK;
}

icpmi_status icpmi_debug_counters(icpmi_handle h, uint64_t out[24])
{
    CHECK_H(h); // (slot 23 is read back from the device)
    if (!out) return ICPMI_ERR_INVALID_ARG;
    for (int i = 0; i < 24; ++i) out[i] = h->h_state->dbg[i];
    // [18] / [19]: index builds served by the incremental insert / from scratch (low word: this handle's registration index; high
    // word: its private raw-frame index, ops.hip: raw_index)
    // (a -DICPMI_NN_TIMING build keeps all 24 slots for the NN kernels' phase clocks -- ADVICE r4)
#ifndef ICPMI_NN_TIMING
    // [10] / [11]: k = 1 matcher, last registration: queries its helper workgroups ran / far-seeded queries that found their defer list full
    out[10] = (uint64_t)h->h_state->defer_served;
    out[11] = (uint64_t)h->h_state->defer_overflow;
    out[14] = (uint64_t)h->merge_fast_epochs; // map-growth epochs served with ONE collective / with the count + ready + points exchanges (ops.hip)
    out[15] = (uint64_t)h->merge_slow_epochs;
    out[16] = (uint64_t)h->oct_respeculated; // octree filter calls whose speculated depth was too shallow (sorted twice; octree.hip)
    out[17] = (uint64_t)h->raw_view_count; // PointDistance searches served by the raw-frame view of the registration index (no second index)
    out[18] = (uint64_t)(uint32_t)h->ins_count | ((uint64_t)(uint32_t)(h->temp_raw ? h->temp_raw->ins_count : 0) << 32);
    out[19] = (uint64_t)(uint32_t)h->full_count | ((uint64_t)(uint32_t)(h->temp_raw ? h->temp_raw->full_count : 0) << 32);
    // (r6) SurfaceNormal passes over the resident map of an append-only update: served by the subset search / over the whole map; points the last pass searched
    out[20] = (uint64_t)h->normals_incremental;
    out[21] = (uint64_t)h->normals_full;
    out[22] = (uint64_t)h->normals_last_searched;
    // changed normals whose copy in the registration index map_patch_normals did not find, since the handle was created: 0, or the index
    // holds stale normals (map_build.hip: patch_normals_kernel; one word read back from the device)
    return map_patch_unplaced(h, &out[23]);
#else
    return ICPMI_OK;
#endif
}

icpmi_status icpmi_debug_index_normals(icpmi_handle h, int64_t m, float* sorted3, float* pn3, int32_t* has_pn)
{
    CHECK_H(h);
    if (m < 1 || !sorted3) { h->last_error = "debug_index_normals: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return map_debug_index_normals(h, m, sorted3, pn3, has_pn);
}

icpmi_status icpmi_debug_last_matches(icpmi_handle h, int64_t n, int32_t k, int32_t* ids, float* d2, float T_used[16])
{
    CHECK_H(h);
    if (n < 1 || k < 1 || !ids || !d2 || !T_used) { h->last_error = "debug_last_matches: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (h->last_match_n == 0) {
        h->last_error = "debug_last_matches: no single registration's matches on this handle (none ran, it failed, or a batch / another call came after it)";
        return ICPMI_ERR_UNSUPPORTED;
    }
    if (n != h->last_match_n || k != h->last_match_k) { h->last_error = "debug_last_matches: n / k differ from the last registration's"; return ICPMI_ERR_INVALID_ARG; }
    // the layout overlap_kernel reads (loop.hip): element e = slot * k + j, slot = the caller's index or -- sorted -- qindex[slot]
    const size_t cnt = (size_t)n * k;
    DevBuf<int> d_ids;
    HIP_TRY(h, d_ids.alloc(cnt));
    icpmi_status s = nn_ids_to_original(h, h->d_sidx, (int64_t)cnt, d_ids);
    if (s != ICPMI_OK) return s;
    std::vector<int> hid(cnt), hq(h->last_match_sorted ? (size_t)n : 0);
    std::vector<float> hd(cnt);
    HIP_TRY(h, hipMemcpyAsync(hid.data(), d_ids, cnt * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(hd.data(), h->d_d2, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (h->last_match_sorted) HIP_TRY(h, hipMemcpyAsync(hq.data(), h->d_qindex, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(T_used, h->d_state->T_prev, 16 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int64_t slot = 0; slot < n; ++slot) {
        const int64_t oi = h->last_match_sorted ? hq[slot] : slot;
        if (oi < 0 || oi >= n) { h->last_error = "debug_last_matches: query index out of range"; return ICPMI_ERR_HIP; }
        for (int j = 0; j < k; ++j) {
            ids[oi * k + j] = hid[slot * k + j];
            d2[oi * k + j] = hd[slot * k + j];
        }
    }
    return ICPMI_OK;
}

icpmi_status icpmi_debug_self_knn(icpmi_handle h, const float* pts4, int64_t m, int32_t k, int32_t* ids, float* d2, uint64_t info[8])
{
    CHECK_H(h);
    if (m < 1 || !pts4 || !ids || !d2) { h->last_error = "debug_self_knn: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_debug_self_knn(h, pts4, m, k, ids, d2, info);
}

icpmi_status icpmi_debug_resident_kth_d2(icpmi_handle h, int64_t m, float* out, int32_t* knn_out)
{
    CHECK_H(h);
    if (m < 1 || !out) { h->last_error = "debug_resident_kth_d2: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_debug_resident_kth_d2(h, m, out, knn_out);
}

icpmi_status icpmi_debug_merge_blocks(icpmi_handle h, const float* pts4, const int64_t* counts, int32_t n_ranks, int64_t stride, float min_dist, int32_t mode,
                                      float* merged_out4, int64_t capacity, int64_t* merged_n, uint8_t* kept_out, int32_t* path_out)
{
    CHECK_H(h);
    if (n_ranks < 1 || n_ranks > 256) { h->last_error = "debug_merge_blocks: n_ranks must be in [1, 256]"; return ICPMI_ERR_INVALID_ARG; }
    if (!counts) { h->last_error = "debug_merge_blocks: counts is null"; return ICPMI_ERR_INVALID_ARG; }
    if (!merged_n || !path_out) { h->last_error = "debug_merge_blocks: merged_n / path_out is null"; return ICPMI_ERR_INVALID_ARG; }
    if (mode != 0 && mode != 1) { h->last_error = "debug_merge_blocks: mode must be 0 or 1"; return ICPMI_ERR_INVALID_ARG; }
    int64_t total = 0;
    for (int r = 0; r < n_ranks; ++r) {
        if (counts[r] < 0) { h->last_error = "debug_merge_blocks: counts[" + std::to_string(r) + "] is negative"; return ICPMI_ERR_INVALID_ARG; }
        if (counts[r] > stride) { h->last_error = "debug_merge_blocks: counts[" + std::to_string(r) + "] is above stride"; return ICPMI_ERR_INVALID_ARG; }
        total += counts[r];
    }
    if (total > 0 && !pts4) { h->last_error = "debug_merge_blocks: pts4 is null"; return ICPMI_ERR_INVALID_ARG; }
    if (capacity < 0 || (total > 0 && capacity > 0 && !merged_out4)) { h->last_error = "debug_merge_blocks: merged_out4 is null (or capacity negative)"; return ICPMI_ERR_INVALID_ARG; }
    return ops_debug_merge_blocks(h, pts4, counts, n_ranks, stride, min_dist, mode, merged_out4, capacity, merged_n, kept_out, path_out);
}

icpmi_status icpmi_debug_keep_sums(icpmi_handle h, int32_t on)
{
    CHECK_H(h);
    if ((on != 0) == (h->d_keep_sums.get() != nullptr)) return ICPMI_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // the cached loop graphs were captured with the other sums_out
    drop_loop_graphs(h);
    if (!on) { HIP_TRY(h, h->d_keep_sums.reset()); return ICPMI_OK; }
    HIP_TRY(h, h->d_keep_sums.alloc(ICPMI_NV));
    HIP_TRY(h, hipMemsetAsync(h->d_keep_sums, 0, ICPMI_NV * sizeof(double), h->stream));
    return ICPMI_OK;
}

icpmi_status icpmi_debug_last_sums(icpmi_handle h, double sums[32], float limits[ICPMI_MAX_OUTLIER], float* robust_scale, float* vt_ratio)
{
    CHECK_H(h);
    if (!sums) { h->last_error = "debug_last_sums: sums is null"; return ICPMI_ERR_INVALID_ARG; }
    if (!h->d_keep_sums.get()) { h->last_error = "debug_last_sums: the pair sums are not kept on this handle (icpmi_debug_keep_sums)"; return ICPMI_ERR_UNSUPPORTED; }
    if (h->last_match_n == 0) {
        h->last_error = "debug_last_sums: no single registration's pair sums on this handle (none ran, it failed, or a batch / another call came after it)";
        return ICPMI_ERR_UNSUPPORTED;
    }
    // (dead iterations behind the stop return before the solve: the block holds the last counted iteration's sums; the state is the mirror
    // loop_run filled for that registration)
    const icpmi_status s = read_back(h, sums, h->d_keep_sums.get(), ICPMI_NV * sizeof(double));
    if (s != ICPMI_OK) return s;
    const IcpState* hs = h->h_state;
    if (limits) for (int f = 0; f < ICPMI_MAX_OUTLIER; ++f) limits[f] = hs->limits[f];
    if (robust_scale) *robust_scale = hs->robust_scale;
    if (vt_ratio) *vt_ratio = hs->vt_ratio;
    return ICPMI_OK;
}

icpmi_status icpmi_get_covariance(icpmi_handle h, float cov[36])
{
    CHECK_H(h);
    if (!cov) { h->last_error = "get_covariance: cov is null"; return ICPMI_ERR_INVALID_ARG; }
    if (!h->cfg.covariance) { h->last_error = "get_covariance: the chain does not ask for a covariance (icpmi_config::covariance)"; return ICPMI_ERR_UNSUPPORTED; }
    if (!h->cov_ready || (h->last_match_n == 0 && !h->cov_kept)) {
        h->last_error = "get_covariance: no covariance of a single registration on this handle (none ran, it failed, or a batch / another call came after it)";
        return ICPMI_ERR_UNSUPPORTED;
    }
    return read_back(h, cov, loop_covariance_out(h), 36 * sizeof(float));
}

icpmi_status icpmi_get_localizability(icpmi_handle h, icpmi_localizability* out)
{
    CHECK_H(h);
    if (!out) { h->last_error = "get_localizability: out is null"; return ICPMI_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    if (h->cfg.degeneracy_threshold == 0.f) { h->last_error = "get_localizability: the chain does not ask for it (icpmi_config::degeneracy_threshold)"; return ICPMI_ERR_UNSUPPORTED; }
    if (!h->degen_ready || !h->d_degen.get()) {
        h->last_error = "get_localizability: no report of a single registration on this handle (none ran, it failed, a batch / multistart call came after it, or the map or the chain changed since)";
        return ICPMI_ERR_UNSUPPORTED;
    }
    const icpmi_status s = read_back(h, out, h->d_degen.get() + ICPMI_DG_OUT, sizeof *out);
    if (s != ICPMI_OK) { memset(out, 0, sizeof *out); return s; }
    for (int r = 0; r < 3; ++r) out->pivot[r] += (double)h->mean[r]; // (the side block keeps c in the centred frame)
    return ICPMI_OK;
}

icpmi_status icpmi_debug_minstd_nth(icpmi_handle h, uint32_t seed, uint32_t n, uint32_t* out)
{
    CHECK_H(h);
    if (!out || n == 0) { h->last_error = "debug_minstd_nth: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    unsigned v = 0;
    const icpmi_status s = ssn_debug_minstd(h, seed, n, &v);
    *out = v;
    return s;
}

icpmi_status icpmi_get_grid_info(icpmi_handle h, float* cell, int32_t dims[3], int64_t* n_cells, int64_t* n_occupied)
{
    if (!h) return ICPMI_ERR_INVALID_ARG;
    if (cell) *cell = h->grid.cell;
    if (dims) { dims[0] = h->grid.nx; dims[1] = h->grid.ny; dims[2] = h->grid.nz; }
    if (n_cells) *n_cells = h->grid.ncells;
    if (n_occupied) *n_occupied = h->n_occupied;
    return ICPMI_OK;
}

icpmi_status icpmi_set_map_dev(icpmi_handle h, const float* d_map4, int64_t m, const float* d_normals3, int32_t* accepted)
{
    CHECK_H(h);
    if (accepted) *accepted = 0;
    if (m < 0 || (m > 0 && !d_map4)) { h->last_error = "set_map: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (m == 0) return ICPMI_OK; // upstream: "Ignoring attempt to setMap with an empty map", returns false
    if (m >= (1ll << 28)) { h->last_error = "set_map: more than 2^28-1 points (match positions carry the pyramid level in their top 4 bits)"; return ICPMI_ERR_UNSUPPORTED; }
    if (h->cfg.minimizer == ICPMI_MIN_POINT_TO_PLANE && !d_normals3) {
        // upstream fails later, inside the minimiser, with InvalidField("normals"); keep the map and
        // let icpmi_register report it
    }
    icpmi_status s = map_build(h, (const float4*)d_map4, m, d_normals3);
    if (s != ICPMI_OK) return s;
    if (accepted) *accepted = 1;
    return ICPMI_OK;
}

icpmi_status icpmi_set_map(icpmi_handle h, const float* map4, int64_t m, const float* normals3, int32_t* accepted)
{
    CHECK_H(h);
    if (accepted) *accepted = 0;
    if (m < 0 || (m > 0 && !map4)) { h->last_error = "set_map: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (m == 0) return ICPMI_OK;
    if (h->d_stage_in.ensure(h, (size_t)m) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(h->d_stage_in, map4, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    if (normals3) {
        if (h->d_stage_n3.ensure(h, (size_t)m * 3) != ICPMI_OK) return ICPMI_ERR_HIP;
        HIP_TRY(h, hipMemcpyAsync(h->d_stage_n3, normals3, (size_t)m * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
    return icpmi_set_map_dev(h, (const float*)h->d_stage_in.get(), m, normals3 ? h->d_stage_n3 : nullptr, accepted);
}

static void identity16(float* T) { for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.f : 0.f; }

// ICPMI_STATS_JSON=<path>: one JSON line per registration with the names libpointmatcher's inspector records for an ICP call
// (IterationsCount, OverlapRatio, ConvergenceDuration) plus the loop's own statistics.  Opened once, appended.
static FILE* stats_json()
{
    static FILE* f = [] { const char* p = getenv("ICPMI_STATS_JSON"); return (p && *p) ? fopen(p, "a") : (FILE*)nullptr; }();
    return f;
}

static void write_stats_json(const icpmi_stats& st, int64_t n, icpmi_status rs)
{
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    fprintf(stats_json(), "{\"IterationsCount\": %d, \"OverlapRatio\": %.9g, \"ConvergenceDuration\": %.9g, \"PointUsedRatio\": %.9g, "
                          "\"PairsUsed\": %lld, \"ReadingPoints\": %lld, \"StopReason\": %d, \"TrimmedLimit\": %.9g, \"Status\": %d}\n",
            st.iterations, (double)st.weighted_point_used_ratio, (double)st.loop_ms * 1e-3, (double)st.point_used_ratio, (long long)st.pairs,
            (long long)n, st.stop_reason, (double)st.trimmed_limit, (int)rs);
    fflush(stats_json());
}

// fields the GenericDescriptor / Robust filters of the chain read on the map
static icpmi_status check_ext_filters(icpmi_ctx* h)
{
    for (int f = 0; f < h->cfg.n_outlier; ++f) {
        const icpmi_outlier& o = h->cfg.outlier[f];
        if (o.type == ICPMI_OUT_GENERICDESCRIPTOR && !(o.iparam & ICPMI_GEN_SOURCE_READING) && !(h->raw_has_scalar && h->m_raw == h->m)) {
            h->last_error = "InvalidField: GenericDescriptorOutlierFilter needs the tracked scalar descriptor on the map (icpmi_set_map_scalar)";
            return ICPMI_ERR_INVALID_ARG;
        }
        if (o.type == ICPMI_OUT_ROBUST && ((o.iparam >> 8) & 15) == ICPMI_DIST_POINT2PLANE && !h->has_normals) {
            h->last_error = "InvalidField: RobustOutlierFilter{distanceType: point2plane} needs the descriptor 'normals' on the map";
            return ICPMI_ERR_MISSING_NORMALS;
        }
    }
    return ICPMI_OK;
}

// the stage entry points carry no reading descriptor: a chain with GenericDescriptorOutlierFilter{source: reading} is served by icpmi_register only
static icpmi_status reject_reading_source(icpmi_ctx* h, const char* who)
{
    for (int f = 0; f < h->cfg.n_outlier; ++f)
        if (h->cfg.outlier[f].type == ICPMI_OUT_GENERICDESCRIPTOR && (h->cfg.outlier[f].iparam & ICPMI_GEN_SOURCE_READING)) {
            h->last_error = std::string(who) + ": GenericDescriptorOutlierFilter{source: reading} is only available inside icpmi_register";
            return ICPMI_ERR_UNSUPPORTED;
        }
    return ICPMI_OK;
}

// KDTreeVarDistMatcher: a row of radii as the matcher kernels take it -- validated (every entry >= 0 or +inf), squared by the expression that
// squares maxDist, and its largest entry (un-squared), the uniform bound of the search
static icpmi_status square_radii(icpmi_ctx* h, const char* who, const float* radii, int64_t n, std::vector<float>& r2, float* max_out)
{
    r2.resize((size_t)n);
    float mx = 0.f;
    for (int64_t i = 0; i < n; ++i) {
        const float r = radii[i];
        if (!(r >= 0.f)) { // (NaN, a negative radius, -inf)
            h->last_error = std::string(who) + ": every radius must be >= 0 or +inf (entry " + std::to_string((long long)i) + ")";
            return ICPMI_ERR_INVALID_ARG;
        }
        mx = r > mx ? r : mx;
        r2[(size_t)i] = squared_radius(r);
    }
    *max_out = mx;
    return ICPMI_OK;
}

// the one bound a search prunes with (make_loop_cfg derives the same three fields from icpmi_config::max_dist)
static void set_search_bound(const icpmi_ctx* h, LoopCfg& lc, float max_dist)
{
    lc.max_dist = max_dist;
    lc.maxr2 = squared_radius(max_dist);
    if (std::isfinite(max_dist) && h->grid.cell > 0.f) {
        const int need = (int)ceilf(max_dist / h->grid.cell) + 1;
        lc.ring_max = need < 16 ? need : 16;
    } else lc.ring_max = 6;
    if (lc.ring_max < 1) lc.ring_max = 1;
}

// the stage entry points that run the handle's matcher carry no radii: a KDTreeVarDistMatcher chain is served by icpmi_register (and icpmi_knn_var)
static icpmi_status reject_var_dist(icpmi_ctx* h, const char* who)
{
    if (!h->cfg.var_dist) return ICPMI_OK;
    h->last_error = std::string(who) + ": KDTreeVarDistMatcher is only available inside icpmi_register and icpmi_knn_var";
    return ICPMI_ERR_UNSUPPORTED;
}

// the side block of the degeneracy-aware solve, before make_loop_cfg looks for it (allocated once, zeroed; never while a stream captures)
static icpmi_status ensure_degen_block(icpmi_ctx* h)
{
    if (h->cfg.degeneracy_threshold == 0.f || h->d_degen.get()) return ICPMI_OK;
    HIP_TRY(h, h->d_degen.alloc(ICPMI_DG_DOUBLES));
    HIP_TRY(h, hipMemsetAsync(h->d_degen.get(), 0, ICPMI_DG_DOUBLES * sizeof(double), h->stream));
    return ICPMI_OK;
}

// What a chain asks of a call that runs its first iteration on a reading, a registration and a residual call alike: its checks, its
// LoopCfg (iters: make_loop_cfg's count) and the one-shot rows the call consumed (have_*), in upstream's order of complaint.
// Out: the LoopCfg, the KDTreeVarDistMatcher row (null without one), whether the chain reads the reading's normals
static icpmi_status chain_setup(icpmi_handle h, int64_t n, const float* d_n3, int64_t have_scalar_n, int64_t have_r2_n, int iters, LoopCfg* lc_out,
                                const float** d_r2row_out, bool* needs_rn_out)
{
    bool needs_rn = false, wants_scalar = false;
    for (int f = 0; f < h->cfg.n_outlier; ++f) {
        const icpmi_outlier& o = h->cfg.outlier[f];
        needs_rn |= o.type == ICPMI_OUT_SURFACENORMAL;
        wants_scalar |= o.type == ICPMI_OUT_GENERICDESCRIPTOR && (o.iparam & ICPMI_GEN_SOURCE_READING);
    }
    *needs_rn_out = needs_rn;
    if (needs_rn && (!d_n3 || !h->has_normals)) {
        h->last_error = "InvalidField: SurfaceNormalOutlierFilter needs 'normals' on both reading and map";
        return ICPMI_ERR_MISSING_NORMALS;
    }
    { const icpmi_status es = check_ext_filters(h); if (es != ICPMI_OK) return es; }
    LoopCfg& lc = *lc_out;
    lc = make_loop_cfg(h, iters);
    // GenericDescriptorOutlierFilter{source: reading}: the row handed over for THIS reading (one shot)
    if (wants_scalar && n > 0 && have_scalar_n != n) {
        h->last_error = "InvalidField: GenericDescriptorOutlierFilter{source: reading} needs the reading's descriptor (icpmi_set_reading_scalar, one row per point)";
        return ICPMI_ERR_INVALID_ARG;
    }
    lc.read_scalar = wants_scalar ? h->d_read_scalar : nullptr;
    // KDTreeVarDistMatcher: the radii handed over for THIS reading (one shot).  The search runs with one bound, the largest radius of the row;
    // the kernels accept per query (nn.hip: RowR2).
    *d_r2row_out = nullptr;
    if (h->cfg.var_dist && n > 0) {
        if (have_r2_n != n) {
            h->last_error = "InvalidField: KDTreeVarDistMatcher needs the reading's maxDistField descriptor (icpmi_set_reading_max_dist, one radius per point)";
            return ICPMI_ERR_INVALID_ARG;
        }
        if (!(h->read_r2_max > 0.f)) { // (the rule of KDTreeMatcher's maxDist, which this bound stands in for)
            h->last_error = "InvalidParameter: KDTreeVarDistMatcher: the largest radius of the row must be > 0 (as maxDist)";
            return ICPMI_ERR_INVALID_ARG;
        }
        set_search_bound(h, lc, h->read_r2_max);
        *d_r2row_out = h->d_read_r2;
    }
    lc.has_read_normals = needs_rn ? 1 : 0;
    if (n == 0) { // upstream: Trimmed / Median throw "no outlier to filter", otherwise "no point to minimize"
        const bool quant = chain_has_quantile(lc);
        h->last_error = quant ? "ConvergenceError: no outlier to filter" : "ConvergenceError: ErrorMinimizer: no point to minimize";
        return quant ? ICPMI_ERR_NO_OUTLIER_TO_FILTER : ICPMI_ERR_NO_POINT_TO_MINIMIZE;
    }
    return ICPMI_OK;
}

// the name of the minimiser an ICPMI_MIN_PLANE_TO_PLANE handle runs, as the user configured it (icpmi_set_plane_pair_model)
static const char* plane_minimizer_name(const icpmi_ctx* h)
{
    return h->plane_model == ICPMI_PLANE_MODEL_SYMMETRIC ? "SymmetricPointToPlaneErrorMinimizer" : "PlaneToPlaneErrorMinimizer";
}

// the entry points that cannot carry the reading's normals do not serve PlaneToPlaneErrorMinimizer (either pair model)
static icpmi_status reject_plane_to_plane(icpmi_ctx* h, const char* who)
{
    if (h->cfg.minimizer != ICPMI_MIN_PLANE_TO_PLANE) return ICPMI_OK;
    h->last_error = std::string(who) + ": " + plane_minimizer_name(h) + " needs the reading's normals, which this entry point cannot carry "
                    "(icpmi_register*, icpmi_minimize_step_normals take them)";
    return ICPMI_ERR_UNSUPPORTED;
}

// The photometric term (icpmi_set_intensity_weight > 0) is served on plain point-to-plane chains by the entry points that run
// the loop's pair sums on ONE reading.  Everything else says so:
// ... the entry points that cannot carry it
static icpmi_status reject_intensity(icpmi_ctx* h, const char* who)
{
    if (!(h->intensity_w > 0.f)) return ICPMI_OK;
    h->last_error = std::string(who) + ": the intensity term (icpmi_set_intensity_weight > 0) is served by icpmi_register*, icpmi_register_prior* and "
                    "icpmi_minimize_step* only; set the weight to 0 for this entry point";
    return ICPMI_ERR_UNSUPPORTED;
}
// ... the chains it is not defined for, then what it needs: the map's channel and the row of THIS reading (have_int_n: what the call consumed).
// On success lc carries both (common.h: LoopCfg::map_gi from make_loop_cfg, read_intensity from here, where n is known).
static icpmi_status intensity_setup(icpmi_ctx* h, const char* who, int64_t n, int64_t have_int_n, LoopCfg* lc)
{
    if (!(h->intensity_w > 0.f)) return ICPMI_OK;
    const icpmi_config& cfg = h->cfg;
    const char* why = nullptr;
    if (cfg.minimizer != ICPMI_MIN_POINT_TO_PLANE) why = "is defined on ICPMI_MIN_POINT_TO_PLANE only";
    else if (cfg.force_2d || cfg.is_2d) why = "is not served with force_2d / is_2d";
    else if (cfg.covariance) why = "is not served with covariance = 1 (Censi's form is derived for the point-to-plane residual alone)";
    else if (cfg.degeneracy_threshold != 0.f) why = "is not served with a degeneracy_threshold (the localizability report is defined on the geometric term)";
    if (why) {
        h->last_error = std::string(who) + ": the intensity term (icpmi_set_intensity_weight > 0) " + why;
        return ICPMI_ERR_UNSUPPORTED;
    }
    if (!map_intensity_ready(h)) {
        h->last_error = "InvalidField: the intensity term needs the map's intensity channel (icpmi_set_map_intensity, after every change of the map)";
        return ICPMI_ERR_INVALID_ARG;
    }
    if (have_int_n != n) {
        h->last_error = "InvalidField: the intensity term needs the reading's intensity (icpmi_set_reading_intensity, one value per point)";
        return ICPMI_ERR_INVALID_ARG;
    }
    lc->read_intensity = h->d_read_scalar.get() + n; // (the intensity row sits n floats behind the GenericDescriptor row in the one buffer)
    return ICPMI_OK;
}

// VoxelMatcher (icpmi_set_voxel_matcher > 0 or icpmi_set_voxel_schedule with a size) is served on plane-to-plane chains with the GICP pair model and no outlier
// filter, by the entry points that carry the reading's normals and run ONE reading.  Everything else says so and names the matcher; nothing
// is served by the nearest-neighbour path in silence.  served = this entry point can run it
static icpmi_status voxel_check(icpmi_ctx* h, const char* who, bool served)
{
    if (!(h->voxel_size > 0.f)) return ICPMI_OK;
    if (!served) {
        h->last_error = std::string(who) + ": the voxel matcher (icpmi_set_voxel_matcher > 0) is served by icpmi_register, icpmi_register_dev, "
                        "icpmi_register_fixed_dev and icpmi_minimize_step_normals only; set the size to 0 for this entry point";
        return ICPMI_ERR_UNSUPPORTED;
    }
    const icpmi_config& cfg = h->cfg;
    const char* why = nullptr;
    if (cfg.minimizer != ICPMI_MIN_PLANE_TO_PLANE) why = "is defined on PlaneToPlaneErrorMinimizer only";
    else if (h->plane_model != ICPMI_PLANE_MODEL_GICP) why = "is not served with the symmetric pair model (SymmetricPointToPlaneErrorMinimizer)";
    else if (cfg.n_outlier > 0) why = "is not served with outlier filters (a pair is a point and the voxel it falls into: there is no match distance to filter on)";
    else if (cfg.var_dist) why = "is not served with KDTreeVarDistMatcher (var_dist)";
    else if (h->intensity_w > 0.f) why = "is not served with the intensity term (icpmi_set_intensity_weight > 0)";
    // (belt and braces: icpmi_set_config refuses the three below for ICPMI_MIN_PLANE_TO_PLANE already, and any other minimiser is answered above)
    else if (cfg.covariance) why = "is not served with covariance = 1";
    else if (cfg.degeneracy_threshold != 0.f) why = "is not served with a degeneracy_threshold";
    else if (cfg.force_2d || cfg.is_2d) why = "is not served with force_2d / is_2d";
    if (why) {
        h->last_error = std::string("InvalidParameter: ") + who + ": the voxel matcher (icpmi_set_voxel_matcher > 0) " + why;
        return ICPMI_ERR_INVALID_ARG;
    }
    return ICPMI_OK;
}

static icpmi_status register_impl(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_n3, int fixed_iters,
                                  float T_out[16], icpmi_stats* stats)
{
    // the one-shot reading rows (icpmi_set_reading_scalar / _sensor_noise) belong to THIS call whatever becomes of it: consumed here, before
    // any early return, so that a registration that bails out cannot leave a stale row armed for the next one
    const int64_t have_scalar_n = h->read_scalar_n, have_noise_n = h->read_noise_n, have_r2_n = h->read_r2_n, have_int_n = h->read_int_n;
    h->read_scalar_n = 0; h->read_noise_n = 0; h->read_r2_n = 0; h->read_int_n = 0;
    h->cov_ready = false; // (loop_run sets it again once the covariance of THIS registration is enqueued)
    h->degen_ready = false; // (... and the localizability report)
    if (!T_out) { h->last_error = "register: T_out is null"; return ICPMI_ERR_INVALID_ARG; }
    if (stats) { memset(stats, 0, sizeof *stats); stats->sensor_noise_overlap = -1.f; } // -1 = "not computed" on EVERY path
    identity16(T_out);
    if (n < 0 || (n > 0 && !d_scan4)) { h->last_error = "register: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    { const icpmi_status vs = voxel_check(h, "register", true); if (vs != ICPMI_OK) return vs; }
    if (h->m <= 0) return ICPMI_OK; // "Ignoring attempt to perform ICP with an empty map" -> identity
    if (n > 0x7fffffff / ICPMI_MAX_K) { h->last_error = "register: too many points"; return ICPMI_ERR_UNSUPPORTED; }
    if (h->cfg.minimizer == ICPMI_MIN_POINT_TO_PLANE && !h->has_normals) {
        h->last_error = "InvalidField: PointToPlaneErrorMinimizer needs the descriptor 'normals' on the map";
        return ICPMI_ERR_MISSING_NORMALS;
    }
    const bool gicp = h->cfg.minimizer == ICPMI_MIN_PLANE_TO_PLANE;
    if (gicp && (!h->has_normals || (n > 0 && !d_n3))) {
        h->last_error = std::string("InvalidField: ") + plane_minimizer_name(h) + " needs the descriptor 'normals' on both reading and map";
        return ICPMI_ERR_MISSING_NORMALS;
    }
    { const icpmi_status ds = ensure_degen_block(h); if (ds != ICPMI_OK) return ds; }
    LoopCfg lc;
    const float* d_r2row = nullptr;
    bool needs_rn = false;
    { const icpmi_status cs = chain_setup(h, n, d_n3, have_scalar_n, have_r2_n, fixed_iters, &lc, &d_r2row, &needs_rn); if (cs != ICPMI_OK) return cs; }
    { const icpmi_status is = intensity_setup(h, "register", n, have_int_n, &lc); if (is != ICPMI_OK) return is; }
    // sensor-noise overlap (icpmi_set_reading_sensor_noise): the noise row is one shot -- this registration consumes it
    // (PointToPointErrorMinimizer::getOverlap() needs `simpleSensorNoise` alone; only the point-to-plane variant also reads the reading's
    // `normals` -- ADVICE r3)
    const bool voxel = voxel_path(h); // (voxel_check passed: the chain is one the voxel matcher serves)
    if (voxel) { const icpmi_status ts = voxel_ensure_table(h, nullptr); if (ts != ICPMI_OK) return ts; } // (before the loop: it allocates and waits)
    if (voxel) ++h->vox_single_regs; // (icpmi_debug_voxel_batch_calls)
    // (a voxel loop leaves no matched pairs behind for the overlap pass: the row is consumed, the overlap stays "not computed")
    const bool sn = !voxel && have_noise_n == n && !lc.ext && !lc.is_2d &&
                    (lc.minimizer == ICPMI_MIN_POINT_TO_POINT || (lc.minimizer == ICPMI_MIN_POINT_TO_PLANE && d_n3));
    lc.sensor_noise = sn ? 1 : 0;
    if (sn && d_n3) lc.has_read_normals = 1;
    if (gicp) lc.has_read_normals = 1; // (the pair sums read them)
    icpmi_stats local;
    if (!stats && stats_json()) stats = &local;
    const icpmi_status rs = loop_run(h, (const float4*)d_scan4, (needs_rn || sn || gicp) ? d_n3 : nullptr, n, lc, d_r2row, fixed_iters > 0, T_out, stats);
    if (stats_json() && stats) write_stats_json(*stats, n, rs);
    return rs;
}

icpmi_status icpmi_set_reading_sensor_noise(icpmi_handle h, const float* noise, int64_t n)
{
    CHECK_H(h);
    h->read_noise_n = 0;
    if (!noise || n <= 0) return ICPMI_OK;
    if (h->d_read_noise.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(h->d_read_noise, noise, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // the caller's buffer is free on return
    h->read_noise_n = n;
    return ICPMI_OK;
}

icpmi_status icpmi_set_reading_scalar(icpmi_handle h, const float* scalar, int64_t n)
{
    CHECK_H(h);
    h->read_scalar_n = 0;
    if (!scalar || n <= 0) return ICPMI_OK;
    if (h->d_read_scalar.ensure_keep(h, 2 * (size_t)n + 1, h->read_int_n == n ? 2 * (size_t)n : 0) != ICPMI_OK) return ICPMI_ERR_HIP; // (row 2: icpmi_set_reading_intensity)
    HIP_TRY(h, hipMemcpyAsync(h->d_read_scalar, scalar, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // the caller's buffer is free on return
    h->read_scalar_n = n;
    return ICPMI_OK;
}

// (the two one-shot rows share d_read_scalar: [0, n) the GenericDescriptor row, [n, 2 n) the intensity row -- a row armed with the same n
//  survives the other setter's growth of the buffer)
icpmi_status icpmi_set_reading_intensity(icpmi_handle h, const float* row, int64_t n)
{
    CHECK_H(h);
    h->read_int_n = 0;
    if (!row || n <= 0) return ICPMI_OK;
    if (h->d_read_scalar.ensure_keep(h, 2 * (size_t)n + 1, h->read_scalar_n == n ? (size_t)n : 0) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(h->d_read_scalar + n, row, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // the caller's buffer is free on return
    h->read_int_n = n;
    return ICPMI_OK;
}

icpmi_status icpmi_set_reading_max_dist(icpmi_handle h, const float* radii, int64_t n)
{
    CHECK_H(h);
    h->read_r2_n = 0;
    if (!radii || n <= 0) return ICPMI_OK;
    std::vector<float> r2;
    float mx = 0.f;
    { const icpmi_status vs = square_radii(h, "set_reading_max_dist", radii, n, r2, &mx); if (vs != ICPMI_OK) return vs; }
    if (h->d_read_r2.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(h->d_read_r2, r2.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // the staging vector is free on return
    h->read_r2_n = n; h->read_r2_max = mx;
    return ICPMI_OK;
}

icpmi_status icpmi_register_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, float T_out[16],
                                icpmi_stats* stats)
{
    CHECK_H(h);
    return register_impl(h, d_scan4, n, d_scan_normals3, 0, T_out, stats);
}

icpmi_status icpmi_register_fixed_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3,
                                      int32_t iterations, float T_out[16], icpmi_stats* stats)
{
    CHECK_H(h);
    if (iterations < 1) { h->last_error = "register_fixed: iterations must be >= 1"; return ICPMI_ERR_INVALID_ARG; }
    return register_impl(h, d_scan4, n, d_scan_normals3, iterations, T_out, stats);
}

// the chains whose kernels take a batch (blockIdx.y = reading): k = 1 on the grid pyramid without a brute-force pass, at most one quantile
// filter, no filter that reads descriptors of the reading, no row of radii per reading
static bool chain_takes_batch(const icpmi_ctx* h)
{
    bool together = h->m > 0 && h->cfg.knn == 1 && (h->cfg.minimizer != ICPMI_MIN_POINT_TO_PLANE || h->has_normals);
    int nquant = 0;
    for (int f = 0; f < h->cfg.n_outlier; ++f) {
        const int t = h->cfg.outlier[f].type;
        if (t == ICPMI_OUT_SURFACENORMAL || t == ICPMI_OUT_GENERICDESCRIPTOR || t == ICPMI_OUT_ROBUST || t == ICPMI_OUT_VARTRIMMEDDIST) together = false;
        if (t == ICPMI_OUT_TRIMMEDDIST || t == ICPMI_OUT_MEDIANDIST) ++nquant;
    }
    if (nquant > 1) together = false;
    if (h->cfg.var_dist) together = false; // (every reading needs its own row of radii)
    if (h->cfg.minimizer == ICPMI_MIN_PLANE_TO_PLANE) together = false; // (... and its own normals)
    if (h->cfg.degeneracy_threshold != 0.f) together = false; // (one side block per handle: the degeneracy-aware solve serves single registrations)
    if (together) {
        const GridParams& top = h->levels.g[h->levels.nlev - 1];
        if (!std::isfinite(h->cfg.max_dist) || (top.cell - top.slack) <= h->cfg.max_dist) together = false; // would need the brute-force pass
    }
    return together;
}

icpmi_status icpmi_register_batch_dev(icpmi_handle h, int32_t batch, const float* const* d_scans4, const int64_t* n, int32_t fixed_iterations,
                                      float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    CHECK_H(h);
    if (batch < 1 || batch > ICPMI_MAX_BATCH || !d_scans4 || !n || !T_out || fixed_iterations < 0) {
        h->last_error = "register_batch: bad arguments (1 <= batch <= 16)"; return ICPMI_ERR_INVALID_ARG;
    }
    for (int b = 0; b < batch; ++b)
        if (n[b] < 0 || (n[b] > 0 && !d_scans4[b])) { h->last_error = "register_batch: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    { const icpmi_status vs = voxel_check(h, "register_batch", false); if (vs != ICPMI_OK) return vs; }
    { const icpmi_status ps = reject_plane_to_plane(h, "register_batch"); if (ps != ICPMI_OK) return ps; }
    { const icpmi_status is = reject_intensity(h, "register_batch"); if (is != ICPMI_OK) return is; }
    // The one-launch-per-iteration path serves the chains whose kernels take a batch: k = 1 on the grid pyramid without a
    // brute-force pass, at most one quantile filter, no filter that reads descriptors of the reading.  Everything else --
    // and empty readings, a handle without a map -- runs the readings one after the other: same results, no sharing.
    bool together = batch > 1 && chain_takes_batch(h);
    for (int b = 0; b < batch; ++b) if (n[b] == 0 || n[b] > 0x7fffffff / ICPMI_MAX_K) together = false;
    if (!together) {
        icpmi_status sb[ICPMI_MAX_BATCH];
        for (int b = 0; b < batch; ++b)
            sb[b] = register_impl(h, d_scans4[b], n[b], nullptr, fixed_iterations, T_out + 16 * b, stats ? stats + b : nullptr);
        h->cov_ready = false; // (no covariance per reading of a batch)
        h->degen_ready = false; // (... and no localizability report)
        return fold_status(h, status, sb, batch, nullptr); // (last_error: what the last reading that failed said)
    }
    if (stats) { memset(stats, 0, sizeof(icpmi_stats) * batch); for (int b = 0; b < batch; ++b) stats[b].sensor_noise_overlap = -1.f; }
    LoopCfg lc = make_loop_cfg(h, fixed_iterations);
    h->cov_ready = false;
    return loop_run_batch(h, batch, d_scans4, n, lc, fixed_iterations > 0, T_out, stats, status);
}

icpmi_status icpmi_register(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, float T_out[16],
                            icpmi_stats* stats)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !scan4)) { h->last_error = "register: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    const float* d_scan = nullptr;
    const float* d_n3 = nullptr;
    if (n > 0 && h->m > 0) {
        if (h->d_stage_in.ensure(h, (size_t)n) != ICPMI_OK) return ICPMI_ERR_HIP;
        HIP_TRY(h, hipMemcpyAsync(h->d_stage_in, scan4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
        d_scan = (const float*)h->d_stage_in.get();
        if (scan_normals3) {
            if (h->d_stage_n3.ensure(h, (size_t)n * 3) != ICPMI_OK) return ICPMI_ERR_HIP;
            HIP_TRY(h, hipMemcpyAsync(h->d_stage_n3, scan_normals3, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
            d_n3 = h->d_stage_n3;
        }
    } else if (n > 0) {
        d_scan = scan4; // no map: never dereferenced
    }
    return register_impl(h, d_scan, n, d_n3, 0, T_out, stats);
}

// icpmi_residual_error*: what the chain asks of a residual call whatever the pose -- its own refusals, then chain_setup.
// have_*: the one-shot rows the call consumed; *kind comes back as 1 or 2
static icpmi_status residual_chain_setup(icpmi_handle h, const char* who, int64_t n, const float* d_n3, int64_t have_scalar_n, int64_t have_r2_n,
                                         int32_t* kind_io, LoopCfg* lc_out, const float** d_r2row_out, bool* needs_rn_out)
{
    int32_t kind = *kind_io;
    if (kind == ICPMI_RES_CHAIN) {
        if (h->cfg.minimizer == ICPMI_MIN_IDENTITY) {
            h->last_error = std::string(who) + ": IdentityErrorMinimizer has no residual (name ICPMI_RES_POINT_TO_POINT or ICPMI_RES_POINT_TO_PLANE)";
            return ICPMI_ERR_UNSUPPORTED;
        }
        kind = h->cfg.minimizer == ICPMI_MIN_POINT_TO_POINT ? ICPMI_RES_POINT_TO_POINT : ICPMI_RES_POINT_TO_PLANE;
    }
    *kind_io = kind;
    if (kind == ICPMI_RES_POINT_TO_PLANE && !h->has_normals) {
        h->last_error = "InvalidField: the point-to-plane residual needs the descriptor 'normals' on the map";
        return ICPMI_ERR_MISSING_NORMALS;
    }
    for (int f = 0; f < h->cfg.n_outlier; ++f) {
        const icpmi_outlier& o = h->cfg.outlier[f];
        if (o.type == ICPMI_OUT_ROBUST && (((o.iparam >> 4) & 15) == ICPMI_SCALE_BERG || (int)o.param2 > 0)) {
            h->last_error = std::string(who) + ": RobustOutlierFilter with scaleEstimator berg or nbIterationForScale > 0 keeps its scale from one "
                            "iteration of a registration to the next: no single pass can answer for it";
            return ICPMI_ERR_UNSUPPORTED;
        }
    }
    return chain_setup(h, n, d_n3, have_scalar_n, have_r2_n, 1, lc_out, d_r2row_out, needs_rn_out);
}

// the pose in the centred frame: [R | t + R mu - mu]
static void centred_pose(const icpmi_ctx* h, const float T[16], float Tc[16])
{
    memcpy(Tc, T, 16 * sizeof(float));
    for (int r = 0; r < 3; ++r)
        Tc[12 + r] = (float)(((double)T[12 + r] + (((double)T[r] * (double)h->mean[0] + (double)T[4 + r] * (double)h->mean[1]) + (double)T[8 + r] * (double)h->mean[2])) -
                             (double)h->mean[r]);
    Tc[3] = Tc[7] = Tc[11] = 0.f; Tc[15] = 1.f;
}

// ... then one matcher pass under T and the reduction (loop_residual)
static icpmi_status residual_impl(icpmi_handle h, const char* who, const float* d_scan4, int64_t n, const float* d_n3, const float T[16], int32_t kind,
                                  icpmi_residual* out)
{
    // the one-shot reading rows belong to THIS call whatever becomes of it, as in register_impl
    const int64_t have_scalar_n = h->read_scalar_n, have_r2_n = h->read_r2_n;
    h->read_scalar_n = 0; h->read_noise_n = 0; h->read_r2_n = 0; h->read_int_n = 0;
    if (!out) { h->last_error = std::string(who) + ": out is null"; return ICPMI_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    out->trimmed_limit = -1.f;
    if (n < 0 || (n > 0 && !d_scan4) || kind < ICPMI_RES_CHAIN || kind > ICPMI_RES_POINT_TO_PLANE) {
        h->last_error = std::string(who) + ": bad arguments"; return ICPMI_ERR_INVALID_ARG;
    }
    if (h->m <= 0) { h->last_error = std::string(who) + ": no map"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffff / ICPMI_MAX_K) { h->last_error = std::string(who) + ": too many points"; return ICPMI_ERR_UNSUPPORTED; }
    float Tid[16];
    identity16(Tid);
    if (!T) T = Tid;
    { const icpmi_status rs = check_rigid(h, T); if (rs != ICPMI_OK) return rs; }
    LoopCfg lc;
    const float* d_r2row = nullptr;
    bool needs_rn = false;
    { const icpmi_status cs = residual_chain_setup(h, who, n, d_n3, have_scalar_n, have_r2_n, &kind, &lc, &d_r2row, &needs_rn); if (cs != ICPMI_OK) return cs; }
    // centring, the padded normals and the tile order of the reading, as a registration's head prepares them
    { const icpmi_status ps = loop_prepare_reading(h, (const float4*)d_scan4, n, needs_rn ? d_n3 : nullptr); if (ps != ICPMI_OK) return ps; }
    float Tc[16];
    centred_pose(h, T, Tc);
    return loop_residual(h, n, lc, Tc, kind, (h->cfg.force_2d != 0 || h->cfg.is_2d != 0) ? 1 : 0, d_r2row, out);
}

// icpmi_residual_error_poses*: the reading's checks once, then every rigid pose -- through the batched launches when the chain takes a
// batch (loop_residual_poses), else one after the other through loop_residual on the reading prepared once
static icpmi_status residual_poses_impl(icpmi_handle h, const char* who, const float* d_scan4, int64_t n, const float* d_n3, const float* T,
                                        int32_t n_poses, int32_t kind, icpmi_residual* out, icpmi_status* status, int32_t* batched)
{
    const int64_t have_scalar_n = h->read_scalar_n, have_r2_n = h->read_r2_n;
    h->read_scalar_n = 0; h->read_noise_n = 0; h->read_r2_n = 0; h->read_int_n = 0;
    if (batched) *batched = 0;
    const bool range_ok = n_poses >= 1 && n_poses <= 4096;
    // zeroed on every whole-call error.  (A count above the limit included: the caller vouches for n_poses entries either way -- a call
    // that succeeds writes as many.)
    const auto zero_all = [&] {
        if (out && n_poses >= 1) memset(out, 0, sizeof(icpmi_residual) * (size_t)n_poses);
        if (status && n_poses >= 1) memset(status, 0, sizeof(icpmi_status) * (size_t)n_poses);
    };
    zero_all();
    if (!out || !T || !range_ok || n < 0 || (n > 0 && !d_scan4) || kind < ICPMI_RES_CHAIN || kind > ICPMI_RES_POINT_TO_PLANE) {
        h->last_error = std::string(who) + ": bad arguments (1 <= n_poses <= 4096)"; return ICPMI_ERR_INVALID_ARG;
    }
    if (h->m <= 0) { h->last_error = std::string(who) + ": no map"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffff / ICPMI_MAX_K) { h->last_error = std::string(who) + ": too many points"; return ICPMI_ERR_UNSUPPORTED; }
    LoopCfg lc;
    const float* d_r2row = nullptr;
    bool needs_rn = false;
    { const icpmi_status cs = residual_chain_setup(h, who, n, d_n3, have_scalar_n, have_r2_n, &kind, &lc, &d_r2row, &needs_rn); if (cs != ICPMI_OK) return cs; }
    const int planar = (h->cfg.force_2d != 0 || h->cfg.is_2d != 0) ? 1 : 0;
    // per pose from here on
    std::vector<icpmi_status> st((size_t)n_poses, ICPMI_OK);
    std::vector<int> live;              // the rigid poses, in the caller's order
    std::vector<float> Tc;              // ... in the centred frame
    for (int p = 0; p < n_poses; ++p) {
        out[p].trimmed_limit = -1.f;
        st[(size_t)p] = check_rigid(h, T + 16 * (size_t)p);
        if (st[(size_t)p] != ICPMI_OK) continue;
        live.push_back(p);
        Tc.resize(Tc.size() + 16);
        centred_pose(h, T + 16 * (size_t)p, Tc.data() + Tc.size() - 16);
    }
    if (!live.empty() && chain_takes_batch(h)) {
        std::vector<icpmi_residual> ro(live.size());
        std::vector<icpmi_status> rs(live.size(), ICPMI_OK);
        for (icpmi_residual& r : ro) { memset(&r, 0, sizeof r); r.trimmed_limit = -1.f; }
        const icpmi_status ls = loop_residual_poses(h, (const float4*)d_scan4, n, lc, Tc.data(), (int)live.size(), kind, planar, ro.data(), rs.data());
        if (ls != ICPMI_OK) { zero_all(); return ls; }
        for (size_t i = 0; i < live.size(); ++i) { out[live[i]] = ro[i]; st[(size_t)live[i]] = rs[i]; }
        if (batched) *batched = (int32_t)live.size();
    } else if (!live.empty()) {
        { const icpmi_status ps = loop_prepare_reading(h, (const float4*)d_scan4, n, needs_rn ? d_n3 : nullptr); if (ps != ICPMI_OK) { zero_all(); return ps; } }
        for (size_t i = 0; i < live.size(); ++i) {
            const icpmi_status s = loop_residual(h, n, lc, Tc.data() + 16 * i, kind, planar, d_r2row, out + live[i]);
            if (s == ICPMI_ERR_HIP) { zero_all(); return s; }
            st[(size_t)live[i]] = s;
        }
    }
    return fold_status(h, status, st.data(), n_poses, (std::string(who) + ": a pose ended with an error (see the per-pose status)").c_str());
}

// a host reading and its optional normals into the operator scratch (slots 8 and 9): the handle's stage buffers stay what
// icpmi_register_prior left them
static icpmi_status stage_in_scratch(icpmi_ctx* h, const float* scan4, int64_t n, const float* normals3, const float** d_scan, const float** d_n3)
{
    float4* d_in = scratch_get<float4>(h, 8, (size_t)n);
    if (!d_in) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(d_in, scan4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    *d_scan = (const float*)d_in;
    if (!normals3) return ICPMI_OK;
    float* d_n = scratch_get<float>(h, 9, (size_t)n * 3);
    if (!d_n) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(d_n, normals3, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    *d_n3 = d_n;
    return ICPMI_OK;
}

icpmi_status icpmi_residual_error_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, const float T[16],
                                      int32_t kind, icpmi_residual* out)
{
    CHECK_H(h);
    return residual_impl(h, "residual_error_dev", d_scan4, n, d_scan_normals3, T, kind, out);
}

icpmi_status icpmi_residual_error(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float T[16],
                                  int32_t kind, icpmi_residual* out)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !scan4)) { h->last_error = "residual_error: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    const float* d_scan = scan4; // (n == 0 or no map: never dereferenced)
    const float* d_n3 = nullptr;
    if (n > 0 && h->m > 0) { const icpmi_status ss = stage_in_scratch(h, scan4, n, scan_normals3, &d_scan, &d_n3); if (ss != ICPMI_OK) return ss; }
    return residual_impl(h, "residual_error", d_scan, n, d_n3, T, kind, out);
}

icpmi_status icpmi_residual_error_staged(icpmi_handle h, const float T[16], int32_t kind, icpmi_residual* out)
{
    CHECK_H(h);
    if (h->scan_map_n <= 0) { h->last_error = "residual_error_staged: no scan staged by icpmi_register_prior"; return ICPMI_ERR_INVALID_ARG; }
    return residual_impl(h, "residual_error_staged", (const float*)h->d_scan_map.get(), h->scan_map_n, nullptr, T, kind, out);
}

icpmi_status icpmi_residual_error_poses_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, const float* T,
                                            int32_t n_poses, int32_t kind, icpmi_residual* out, icpmi_status* status, int32_t* batched)
{
    CHECK_H(h);
    return residual_poses_impl(h, "residual_error_poses_dev", d_scan4, n, d_scan_normals3, T, n_poses, kind, out, status, batched);
}

icpmi_status icpmi_residual_error_poses(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float* T,
                                        int32_t n_poses, int32_t kind, icpmi_residual* out, icpmi_status* status, int32_t* batched)
{
    CHECK_H(h);
    const auto zero_all = [&] { // (a whole-call error leaves out and status zeroed: these returns come before residual_poses_impl does it)
        if (out && n_poses >= 1) memset(out, 0, sizeof(icpmi_residual) * (size_t)n_poses);
        if (status && n_poses >= 1) memset(status, 0, sizeof(icpmi_status) * (size_t)n_poses);
        if (batched) *batched = 0;
    };
    const float* d_scan = scan4; // (n == 0, no map or bad arguments: never dereferenced)
    const float* d_n3 = nullptr;
    if (n > 0 && scan4 && h->m > 0) { // once for all poses
        const icpmi_status ss = stage_in_scratch(h, scan4, n, scan_normals3, &d_scan, &d_n3);
        if (ss != ICPMI_OK) { zero_all(); return ss; }
    }
    return residual_poses_impl(h, "residual_error_poses", d_scan, n, d_n3, T, n_poses, kind, out, status, batched);
}

icpmi_status icpmi_register_multistart_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* priors, int32_t n_starts,
                                           int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    CHECK_H(h);
    if (n_starts < 1 || n_starts > ICPMI_MAX_BATCH || n < 0 || (n > 0 && !d_scan4) || !priors || !T_out || fixed_iterations < 0) {
        h->last_error = "register_multistart: bad arguments (1 <= n_starts <= 16)"; return ICPMI_ERR_INVALID_ARG;
    }
    { const icpmi_status vs = voxel_check(h, "register_multistart", false); if (vs != ICPMI_OK) return vs; }
    { const icpmi_status ps = reject_plane_to_plane(h, "register_multistart"); if (ps != ICPMI_OK) return ps; }
    { const icpmi_status is = reject_intensity(h, "register_multistart"); if (is != ICPMI_OK) return is; }
    h->scan_map_n = 0; // (the slices below reuse the stage of icpmi_register_prior: nothing is left staged)
    const int64_t NS = (n + 63) / 64 * 64;
    if (h->d_scan_map.ensure(h, (size_t)NS * n_starts + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    icpmi_status st[ICPMI_MAX_BATCH];
    int idx[ICPMI_MAX_BATCH], nlive = 0;
    for (int s = 0; s < n_starts; ++s) {
        identity16(T_out + 16 * s);
        if (stats) { memset(stats + s, 0, sizeof(icpmi_stats)); stats[s].sensor_noise_overlap = -1.f; }
        st[s] = check_rigid(h, priors + 16 * s);
        if (st[s] == ICPMI_OK) idx[nlive++] = s;
    }
    if (nlive > 1 && n > 0 && n <= 0x7fffffff / ICPMI_MAX_K && chain_takes_batch(h)) {
        // one slice per start, one loop for all of them
        const float* ptrs[ICPMI_MAX_BATCH];
        int64_t ns[ICPMI_MAX_BATCH];
        for (int i = 0; i < nlive; ++i) {
            float4* slice = h->d_scan_map.get() + (size_t)i * NS;
            const icpmi_status ts = ops_transform_dev(h, priors + 16 * idx[i], (const float4*)d_scan4, n, slice); // Mapper.cpp:197, once per start
            if (ts != ICPMI_OK) return ts;
            ptrs[i] = (const float*)slice; ns[i] = n;
        }
        float Tl[16 * ICPMI_MAX_BATCH];
        icpmi_stats sl[ICPMI_MAX_BATCH];
        icpmi_status stl[ICPMI_MAX_BATCH];
        const icpmi_status bs = icpmi_register_batch_dev(h, nlive, ptrs, ns, fixed_iterations, Tl, sl, stl);
        if (bs != ICPMI_OK) return bs;
        for (int i = 0; i < nlive; ++i) {
            memcpy(T_out + 16 * idx[i], Tl + 16 * i, 16 * sizeof(float));
            if (stats) stats[idx[i]] = sl[i];
            st[idx[i]] = stl[i];
        }
    } else {
        // a chain the batch does not serve: start after start through the ONE buffer icpmi_register_prior_dev uses, so that the loop's
        // cached graphs (keyed by the scan's address) serve every start
        for (int i = 0; i < nlive; ++i) {
            const int s = idx[i];
            st[s] = ops_transform_dev(h, priors + 16 * s, (const float4*)d_scan4, n, h->d_scan_map);
            if (st[s] == ICPMI_OK) st[s] = register_impl(h, (const float*)h->d_scan_map.get(), n, nullptr, fixed_iterations, T_out + 16 * s, stats ? stats + s : nullptr);
            if (st[s] == ICPMI_ERR_HIP) return st[s];
        }
    }
    h->cov_ready = false; // (no covariance per start, as after any batch)
    h->degen_ready = false;
    return fold_status(h, status, st, n_starts, "register_multistart: a start ended with an error (see the per-start status)");
}

icpmi_status icpmi_register_multistart(icpmi_handle h, const float* scan4, int64_t n, const float* priors, int32_t n_starts,
                                       int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !scan4)) { h->last_error = "register_multistart: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0) { // one upload, as icpmi_register_prior
        if (h->d_stage_in.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        HIP_TRY(h, hipMemcpyAsync(h->d_stage_in, scan4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    }
    return icpmi_register_multistart_dev(h, n > 0 ? (const float*)h->d_stage_in.get() : nullptr, n, priors, n_starts, fixed_iterations, T_out, stats, status);
}

// ---- many readings, or many starts, on the voxel path --------------------------
// What the whole call is refused for, before anything is enqueued: a handle off the voxel path, then everything voxel_check refuses for
// a single registration, in its words.
static icpmi_status voxel_batch_check(icpmi_ctx* h, const char* who)
{
    if (!(h->voxel_size > 0.f)) {
        h->last_error = std::string(who) + ": the handle is not on the voxel path (icpmi_set_voxel_matcher or icpmi_set_voxel_schedule with a size > 0)";
        return ICPMI_ERR_INVALID_ARG;
    }
    return voxel_check(h, "register", true);
}

// the report of a registration that went through register_impl, as member b's
static void voxel_batch_report_from_single(icpmi_ctx* h, int b)
{
    for (int i = 0; i < 1 + 3 * ICPMI_MAX_VOXEL_LEVELS; ++i) h->vox_batch_report[b][i] = h->vox_levels >= 2 ? h->vox_report[i] : 0;
}

// the members of a batch, checked: through the one loop, or -- a batch of one, an empty member -- one after the other
static icpmi_status voxel_batch_impl(icpmi_handle h, const char* who, int batch, const float* const* d_scans4, const int64_t* n,
                                     const float* const* d_n3, int fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    h->read_scalar_n = 0; h->read_noise_n = 0; h->read_r2_n = 0; h->read_int_n = 0; // (the one-shot reading rows belong to this call)
    h->cov_ready = false; h->degen_ready = false; h->last_match_n = 0; h->cov_kept = false;
    h->scan_map_n = 0;
    h->vox_batch_members = 0;
    for (int b = 0; b < batch; ++b) {
        identity16(T_out + 16 * b);
        if (stats) { memset(stats + b, 0, sizeof(icpmi_stats)); stats[b].sensor_noise_overlap = -1.f; }
        if (status) status[b] = ICPMI_OK;
    }
    { const icpmi_status vs = voxel_batch_check(h, who); if (vs != ICPMI_OK) return vs; }
    for (int b = 0; b < batch; ++b)
        if (n[b] > 0 && !d_n3[b]) {
            h->last_error = std::string("InvalidField: ") + plane_minimizer_name(h) + " needs the descriptor 'normals' on both reading and map";
            return ICPMI_ERR_MISSING_NORMALS;
        }
    memset(h->vox_batch_report, 0, sizeof h->vox_batch_report);
    if (h->m <= 0) { h->vox_batch_members = batch; return ICPMI_OK; } // (an empty map: identities, as a single registration answers; empty reports)
    bool together = batch > 1;
    for (int b = 0; b < batch; ++b) if (n[b] == 0 || n[b] > 0x7fffffff / ICPMI_MAX_K) together = false;
    if (!together) {
        icpmi_status sb[ICPMI_MAX_BATCH];
        for (int b = 0; b < batch; ++b) {
            sb[b] = register_impl(h, d_scans4[b], n[b], d_n3[b], fixed_iterations, T_out + 16 * b, stats ? stats + b : nullptr);
            if (sb[b] == ICPMI_ERR_HIP) return sb[b];
            voxel_batch_report_from_single(h, b);
        }
        h->vox_batch_members = batch;
        h->last_match_n = 0; h->cov_ready = false; h->degen_ready = false;
        return fold_status(h, status, sb, batch, nullptr); // (last_error: what the last reading that failed said)
    }
    { const icpmi_status ts = voxel_ensure_table(h, nullptr); if (ts != ICPMI_OK) return ts; } // (before the loop: both allocate and wait)
    { const icpmi_status ts = voxel_ensure_batch_block(h); if (ts != ICPMI_OK) return ts; }
    LoopCfg lc = make_loop_cfg(h, fixed_iterations);
    lc.has_read_normals = 1; // (as register_impl leaves the chain of a plane-to-plane handle)
    ++h->vox_batch_loops; h->vox_batch_loop_members += batch;
    const icpmi_status rs = loop_run_voxel_batch(h, batch, d_scans4, n, d_n3, lc, T_out, stats, status);
    if (rs != ICPMI_ERR_HIP) h->vox_batch_members = batch;
    return rs;
}

icpmi_status icpmi_voxel_register_batch_dev(icpmi_handle h, int32_t batch, const float* const* d_scans4, const int64_t* n,
                                            const float* const* d_scan_normals3, int32_t fixed_iterations, float* T_out, icpmi_stats* stats,
                                            icpmi_status* status)
{
    CHECK_H(h);
    if (batch < 1 || batch > ICPMI_MAX_BATCH || !d_scans4 || !n || !d_scan_normals3 || !T_out || fixed_iterations < 0) {
        h->last_error = "voxel_register_batch: bad arguments (1 <= batch <= 16)"; return ICPMI_ERR_INVALID_ARG;
    }
    for (int b = 0; b < batch; ++b)
        if (n[b] < 0 || (n[b] > 0 && !d_scans4[b])) {
            for (int i = 0; i < batch; ++i) identity16(T_out + 16 * i);
            h->last_error = "voxel_register_batch: bad arguments"; return ICPMI_ERR_INVALID_ARG;
        }
    return voxel_batch_impl(h, "voxel_register_batch", batch, d_scans4, n, d_scan_normals3, fixed_iterations, T_out, stats, status);
}

// ... for readings on the host: every reading and its normals uploaded once into the operator scratch (slots 8 and 9), then the call above
icpmi_status icpmi_voxel_register_batch(icpmi_handle h, int32_t batch, const float* const* scans4, const int64_t* n, const float* const* scan_normals3,
                                        int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    CHECK_H(h);
    if (batch < 1 || batch > ICPMI_MAX_BATCH || !scans4 || !n || !scan_normals3 || !T_out || fixed_iterations < 0) {
        h->last_error = "voxel_register_batch: bad arguments (1 <= batch <= 16)"; return ICPMI_ERR_INVALID_ARG;
    }
    const float* dp[ICPMI_MAX_BATCH]; const float* dn[ICPMI_MAX_BATCH];
    size_t total = 0;
    bool bad = false;
    for (int b = 0; b < batch; ++b) { bad |= n[b] < 0 || (n[b] > 0 && !scans4[b]); if (!bad) total += (size_t)n[b]; }
    const bool stage = !bad && h->m > 0 && h->voxel_size > 0.f && total > 0; // (otherwise the call below answers before it reads a reading)
    float4* d_in = stage ? scratch_get<float4>(h, 8, total) : nullptr;
    float* d_n = stage ? scratch_get<float>(h, 9, 3 * total) : nullptr;
    if (stage && (!d_in || !d_n)) return ICPMI_ERR_HIP;
    size_t off = 0;
    for (int b = 0; b < batch; ++b) {
        dp[b] = scans4[b]; dn[b] = scan_normals3[b];
        if (!stage || n[b] <= 0) continue;
        HIP_TRY(h, hipMemcpyAsync(d_in + off, scans4[b], (size_t)n[b] * sizeof(float4), hipMemcpyHostToDevice, h->stream));
        dp[b] = (const float*)(d_in + off);
        if (scan_normals3[b]) {
            HIP_TRY(h, hipMemcpyAsync(d_n + 3 * off, scan_normals3[b], (size_t)n[b] * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
            dn[b] = d_n + 3 * off;
        }
        off += (size_t)n[b];
    }
    return icpmi_voxel_register_batch_dev(h, batch, dp, n, dn, fixed_iterations, T_out, stats, status);
}

icpmi_status icpmi_voxel_register_multistart_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, const float* priors,
                                                 int32_t n_starts, int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    CHECK_H(h);
    if (n_starts < 1 || n_starts > ICPMI_MAX_BATCH || n < 0 || (n > 0 && !d_scan4) || !priors || !T_out || fixed_iterations < 0) {
        h->last_error = "voxel_register_multistart: bad arguments (1 <= n_starts <= 16)"; return ICPMI_ERR_INVALID_ARG;
    }
    h->vox_batch_members = 0;
    for (int s = 0; s < n_starts; ++s) {
        identity16(T_out + 16 * s);
        if (stats) { memset(stats + s, 0, sizeof(icpmi_stats)); stats[s].sensor_noise_overlap = -1.f; }
        if (status) status[s] = ICPMI_OK;
    }
    { const icpmi_status vs = voxel_batch_check(h, "voxel_register_multistart"); if (vs != ICPMI_OK) return vs; }
    if (n > 0 && !d_scan_normals3) {
        h->last_error = std::string("InvalidField: ") + plane_minimizer_name(h) + " needs the descriptor 'normals' on both reading and map";
        return ICPMI_ERR_MISSING_NORMALS;
    }
    icpmi_status st[ICPMI_MAX_BATCH];
    int idx[ICPMI_MAX_BATCH], nlive = 0;
    for (int s = 0; s < n_starts; ++s) {
        st[s] = check_rigid(h, priors + 16 * s);
        if (st[s] == ICPMI_OK) idx[nlive++] = s;
    }
    if (h->m <= 0) nlive = 0; // (an empty map: identities, as a single registration answers; the reading is not touched)
    // every live start into slices of its own, points and normals (the stage of icpmi_register_prior and an operator scratch: nothing is
    // left staged), then the slices through the batch
    h->scan_map_n = 0;
    const int64_t NS = (n + 63) / 64 * 64;
    float* d_nslices = nullptr;
    if (n > 0 && nlive > 0) {
        if (h->d_scan_map.ensure(h, (size_t)NS * nlive + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        d_nslices = scratch_get<float>(h, 19, (size_t)3 * NS * nlive + 3);
        if (!d_nslices) return ICPMI_ERR_HIP;
    }
    const float* ptrs[ICPMI_MAX_BATCH]; const float* nptrs[ICPMI_MAX_BATCH];
    int64_t ns[ICPMI_MAX_BATCH];
    for (int i = 0; i < nlive; ++i) {
        float4* slice = n > 0 ? h->d_scan_map.get() + (size_t)i * NS : nullptr;
        float* nslice = n > 0 ? d_nslices + (size_t)3 * i * NS : nullptr;
        const icpmi_status ts = ops_transform_normals_dev(h, priors + 16 * idx[i], (const float4*)d_scan4, d_scan_normals3, n, slice, nslice);
        if (ts != ICPMI_OK) return ts;
        ptrs[i] = (const float*)slice; nptrs[i] = nslice; ns[i] = n;
    }
    int32_t rep[ICPMI_MAX_BATCH][1 + 3 * ICPMI_MAX_VOXEL_LEVELS];
    memset(rep, 0, sizeof rep);
    if (nlive > 0) {
        float Tl[16 * ICPMI_MAX_BATCH];
        icpmi_stats sl[ICPMI_MAX_BATCH];
        icpmi_status stl[ICPMI_MAX_BATCH];
        const icpmi_status bs = voxel_batch_impl(h, "voxel_register_multistart", nlive, ptrs, ns, nptrs, fixed_iterations, Tl, sl, stl);
        if (bs != ICPMI_OK) return bs;
        for (int i = 0; i < nlive; ++i) {
            memcpy(T_out + 16 * idx[i], Tl + 16 * i, 16 * sizeof(float));
            if (stats) stats[idx[i]] = sl[i];
            st[idx[i]] = stl[i];
            memcpy(rep[idx[i]], h->vox_batch_report[i], sizeof rep[0]);
        }
    } else {
        h->read_scalar_n = 0; h->read_noise_n = 0; h->read_r2_n = 0; h->read_int_n = 0;
        h->cov_ready = false; h->degen_ready = false; h->last_match_n = 0; h->cov_kept = false;
    }
    memcpy(h->vox_batch_report, rep, sizeof rep); // (by start: a start that was not launched reports nothing)
    h->vox_batch_members = n_starts;
    return fold_status(h, status, st, n_starts, "voxel_register_multistart: a start ended with an error (see the per-start status)");
}

icpmi_status icpmi_voxel_register_multistart(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float* priors,
                                             int32_t n_starts, int32_t fixed_iterations, float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !scan4)) { h->last_error = "voxel_register_multistart: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    const float* d_scan = scan4; // (n == 0, no map or a call that is refused: never dereferenced)
    const float* d_n3 = scan_normals3;
    if (n > 0 && h->m > 0 && h->voxel_size > 0.f && n_starts >= 1 && n_starts <= ICPMI_MAX_BATCH) { // one upload of the scan and its normals
        d_n3 = nullptr;
        const icpmi_status ss = stage_in_scratch(h, scan4, n, scan_normals3, &d_scan, &d_n3);
        if (ss != ICPMI_OK) return ss;
    }
    return icpmi_voxel_register_multistart_dev(h, d_scan, n, d_n3, priors, n_starts, fixed_iterations, T_out, stats, status);
}

icpmi_status icpmi_get_voxel_batch_report(icpmi_handle h, int32_t member, int32_t* levels, int32_t iterations[4], int32_t pairs_first[4],
                                          int32_t pairs_last[4])
{
    CHECK_H(h);
    if (!levels || !iterations || !pairs_first || !pairs_last) { h->last_error = "get_voxel_batch_report: null argument"; return ICPMI_ERR_INVALID_ARG; }
    if (h->vox_levels < 2) { h->last_error = "get_voxel_batch_report: the handle has no schedule of two or more voxel sizes (icpmi_set_voxel_schedule)"; return ICPMI_ERR_INVALID_ARG; }
    if (member < 0 || member >= h->vox_batch_members) { h->last_error = "get_voxel_batch_report: the last batch or multistart had no such member"; return ICPMI_ERR_INVALID_ARG; }
    const int32_t* r = h->vox_batch_report[member];
    *levels = r[0];
    for (int l = 0; l < ICPMI_MAX_VOXEL_LEVELS; ++l) {
        iterations[l] = r[1 + l];
        pairs_first[l] = r[1 + ICPMI_MAX_VOXEL_LEVELS + l];
        pairs_last[l] = r[1 + 2 * ICPMI_MAX_VOXEL_LEVELS + l];
    }
    return ICPMI_OK;
}

// test seam: [0] loops run by the voxel batch, [1] members they carried, [2] single registrations on the voxel path
icpmi_status icpmi_debug_voxel_batch_calls(icpmi_handle h, int64_t out[3])
{
    if (!h || !out) return ICPMI_ERR_INVALID_ARG;
    out[0] = h->vox_batch_loops; out[1] = h->vox_batch_loop_members; out[2] = h->vox_single_regs;
    return ICPMI_OK;
}

icpmi_status icpmi_transform(icpmi_handle h, const float T[16], const float* in4, int64_t n, float* out4, const float* in_normals3,
                             float* out_normals3)
{
    CHECK_H(h);
    if (!T || n < 0 || (n > 0 && (!in4 || !out4))) { h->last_error = "transform: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_transform(h, T, in4, n, out4, in_normals3, out_normals3);
}

// icpmi_knn (radii == nullptr: max_dist for every query) and icpmi_knn_var (radii: one per query; the search runs with their maximum)
static icpmi_status knn_impl(icpmi_handle h, const float* q4, int64_t n, int32_t k, float max_dist, const float* radii, int32_t allow_self,
                             int32_t* ids, float* d2)
{
    if (n < 0 || k < 1 || k > ICPMI_MAX_K || (n > 0 && (!q4 || !ids || !d2)) || (!radii && !(max_dist > 0.f))) {
        h->last_error = "knn: bad arguments"; return ICPMI_ERR_INVALID_ARG;
    }
    if (n == 0) return ICPMI_OK;
    std::vector<float> r2;
    if (radii) {
        const icpmi_status vs = square_radii(h, "knn_var", radii, n, r2, &max_dist);
        if (vs != ICPMI_OK) return vs;
    }
    if (h->m <= 0 || !(max_dist > 0.f)) { // (no map; a row of zeros: no query accepts anything)
        for (int64_t i = 0; i < n * k; ++i) { ids[i] = -1; d2[i] = INFINITY; }
        return ICPMI_OK;
    }
    const size_t cnt = (size_t)n * k + 1;
    if (h->d_reading.ensure(h, (size_t)n + 1) != ICPMI_OK || h->d_sidx.ensure(h, cnt) != ICPMI_OK ||
        h->d_d2.ensure(h, cnt) != ICPMI_OK || h->d_hard.ensure(h, (size_t)n + 1) != ICPMI_OK)
        return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(h->d_reading, q4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_state, 0, sizeof(IcpState), h->stream));
    DevBuf<float> d_row; // (its own block: a row armed by icpmi_set_reading_max_dist stays armed)
    NnRequest req; // stage call: the caller's order, no quantile selection behind it
    if (radii) {
        HIP_TRY(h, d_row.alloc((size_t)n));
        HIP_TRY(h, hipMemcpyAsync(d_row, r2.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
        req.r2row = d_row;
    }
    if (k == 1) {
        icpmi_status ss = sort_queries(h, h->d_reading, n);
        if (ss != ICPMI_OK) return ss;
    } else {
        h->qsorted_n = -1; h->qsorted_src = nullptr;
    }
    LoopCfg lc = make_loop_cfg(h, 1);
    lc.k = k;
    set_search_bound(h, lc, max_dist); // (m > 0 here, and every index that was built has grid.cell > 0: map_build.hip clamp_cell)
    icpmi_status s = nn_launch_k(h, req, h->d_reading, n, nullptr, lc, allow_self, h->d_sidx, h->d_d2, h->d_state);
    if (s != ICPMI_OK) return s;
    DevBuf<int> d_ids;
    HIP_TRY(h, d_ids.alloc((size_t)n * k));
    s = nn_ids_to_original(h, h->d_sidx, n * k, d_ids);
    hipError_t e = hipSuccess;
    if (s == ICPMI_OK) {
        e = hipMemcpyAsync(ids, d_ids, (size_t)n * k * sizeof(int), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d2, h->d_d2, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (s != ICPMI_OK) return s;
    HIP_TRY(h, e);
    return ICPMI_OK;
}

icpmi_status icpmi_knn(icpmi_handle h, const float* q4, int64_t n, int32_t k, float max_dist, int32_t allow_self, int32_t* ids,
                       float* d2)
{
    CHECK_H(h);
    return knn_impl(h, q4, n, k, max_dist, nullptr, allow_self, ids, d2);
}

icpmi_status icpmi_knn_var(icpmi_handle h, const float* q4, int64_t n, int32_t k, const float* radii, int32_t allow_self, int32_t* ids,
                           float* d2)
{
    CHECK_H(h);
    if (!radii) { h->last_error = "knn_var: radii is null"; return ICPMI_ERR_INVALID_ARG; }
    return knn_impl(h, q4, n, k, 0.f, radii, allow_self, ids, d2);
}

icpmi_status icpmi_outlier_weights(icpmi_handle h, const float* d2, const int32_t* ids, int32_t k, int64_t n,
                                   const float* read_normals3, float* weights, float* limit_out)
{
    CHECK_H(h);
    if (k < 1 || n < 0 || (n > 0 && (!d2 || !weights))) { h->last_error = "outlier_weights: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (n == 0) return ICPMI_OK;
    { const icpmi_status rs = reject_reading_source(h, "outlier_weights"); if (rs != ICPMI_OK) return rs; }
    LoopCfg lc = make_loop_cfg(h, 1);
    return loop_outlier_weights(h, lc, d2, ids, k, n, read_normals3, weights, limit_out);
}

// icpmi_minimize_step (read_normals3 == nullptr) and icpmi_minimize_step_normals
static icpmi_status minimize_step_impl(icpmi_handle h, const float* reading4, int64_t n, const float* read_normals3, const float* T_iter,
                                       float T_step[16], double sums[32], icpmi_stats* stats)
{
    const int64_t have_int_n = h->read_int_n; // (the one-shot intensity row belongs to THIS call whatever becomes of it)
    h->read_int_n = 0;
    if (n <= 0 || !reading4) { h->last_error = "minimize_step: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    { const icpmi_status vs = voxel_check(h, "minimize_step", true); if (vs != ICPMI_OK) return vs; }
    { const icpmi_status es = check_ext_filters(h); if (es != ICPMI_OK) return es; }
    { const icpmi_status rs = reject_reading_source(h, "minimize_step"); if (rs != ICPMI_OK) return rs; }
    { const icpmi_status rs = reject_var_dist(h, "minimize_step"); if (rs != ICPMI_OK) return rs; }
    if (h->m <= 0) { h->last_error = "minimize_step: no map"; return ICPMI_ERR_INVALID_ARG; }
    if (h->cfg.minimizer == ICPMI_MIN_POINT_TO_PLANE && !h->has_normals) {
        h->last_error = "InvalidField: PointToPlaneErrorMinimizer needs the descriptor 'normals' on the map";
        return ICPMI_ERR_MISSING_NORMALS;
    }
    if (h->cfg.minimizer == ICPMI_MIN_PLANE_TO_PLANE && (!h->has_normals || !read_normals3)) {
        h->last_error = std::string("InvalidField: ") + plane_minimizer_name(h) + " needs the descriptor 'normals' on both reading and map";
        return ICPMI_ERR_MISSING_NORMALS;
    }
    if (stats) { memset(stats, 0, sizeof *stats); stats->sensor_noise_overlap = -1.f; }
    if (voxel_path(h)) { const icpmi_status ts = voxel_ensure_table(h, nullptr); if (ts != ICPMI_OK) return ts; }
    if (h->d_reading.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(h->d_reading, reading4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    // d_reading has new contents: a tile-sorted copy of what was there before (an icpmi_knn with the same n) must not be searched in
    // its place (r3: tests/test_gpu_golden.py found the step computed on the previous call's queries)
    h->qsorted_n = -1; h->qsorted_src = nullptr;
    { const icpmi_status ds = ensure_degen_block(h); if (ds != ICPMI_OK) return ds; }
    LoopCfg lc = make_loop_cfg(h, 1);
    for (int f = 0; f < lc.n_out; ++f)
        if (lc.out_type[f] == ICPMI_OUT_SURFACENORMAL) {
            if (!read_normals3) { h->last_error = "minimize_step: SurfaceNormal filter needs icpmi_register"; return ICPMI_ERR_UNSUPPORTED; }
            if (!h->has_normals) { h->last_error = "InvalidField: SurfaceNormalOutlierFilter needs 'normals' on both reading and map"; return ICPMI_ERR_MISSING_NORMALS; }
        }
    { const icpmi_status is = intensity_setup(h, "minimize_step", n, have_int_n, &lc); if (is != ICPMI_OK) return is; }
    if (read_normals3) {
        const icpmi_status us = loop_upload_read_normals(h, read_normals3, n);
        if (us != ICPMI_OK) return us;
        lc.has_read_normals = 1;
    }
    return loop_single_step(h, n, lc, T_iter, T_step, sums, stats);
}

icpmi_status icpmi_minimize_step(icpmi_handle h, const float* reading4, int64_t n, const float* T_iter, float T_step[16],
                                 double sums[32], icpmi_stats* stats)
{
    CHECK_H(h);
    { const icpmi_status vs = voxel_check(h, "minimize_step", false); if (vs != ICPMI_OK) return vs; }
    { const icpmi_status ps = reject_plane_to_plane(h, "minimize_step"); if (ps != ICPMI_OK) return ps; }
    return minimize_step_impl(h, reading4, n, nullptr, T_iter, T_step, sums, stats);
}

icpmi_status icpmi_minimize_step_normals(icpmi_handle h, const float* reading4, int64_t n, const float* read_normals3, const float* T_iter,
                                         float T_step[16], double sums[32], icpmi_stats* stats)
{
    CHECK_H(h);
    return minimize_step_impl(h, reading4, n, read_normals3, T_iter, T_step, sums, stats);
}

icpmi_status icpmi_set_plane_epsilon(icpmi_handle h, float eps)
{
    CHECK_H(h);
    if (!std::isfinite(eps) || !(eps > 0.f) || eps > 1.f) { h->last_error = "set_plane_epsilon: epsilon must be finite and in (0, 1]"; return ICPMI_ERR_INVALID_ARG; }
    h->plane_eps = eps; // (no graph to drop: make_loop_cfg puts it into the LoopCfg, which loop_sig hashes)
    return ICPMI_OK;
}

icpmi_status icpmi_get_plane_epsilon(icpmi_handle h, float* eps)
{
    CHECK_H(h);
    if (!eps) { h->last_error = "get_plane_epsilon: eps is null"; return ICPMI_ERR_INVALID_ARG; }
    *eps = h->plane_eps;
    return ICPMI_OK;
}

icpmi_status icpmi_set_plane_pair_model(icpmi_handle h, int32_t model)
{
    CHECK_H(h);
    if (model != ICPMI_PLANE_MODEL_GICP && model != ICPMI_PLANE_MODEL_SYMMETRIC) {
        h->last_error = "set_plane_pair_model: model must be ICPMI_PLANE_MODEL_GICP or ICPMI_PLANE_MODEL_SYMMETRIC"; return ICPMI_ERR_INVALID_ARG;
    }
    h->plane_model = model; // (no graph to drop: make_loop_cfg puts it into the LoopCfg, which loop_sig hashes)
    return ICPMI_OK;
}

icpmi_status icpmi_get_plane_pair_model(icpmi_handle h, int32_t* model)
{
    CHECK_H(h);
    if (!model) { h->last_error = "get_plane_pair_model: model is null"; return ICPMI_ERR_INVALID_ARG; }
    *model = h->plane_model;
    return ICPMI_OK;
}

// the handle's schedule becomes sizes[0..n) (validated by the caller); a level whose size stays keeps its table
static void voxel_apply_schedule(icpmi_ctx* h, const float* sizes, int n)
{
    for (int l = 0; l < ICPMI_MAX_VOXEL_LEVELS; ++l) h->vox_sizes[l] = l < n ? sizes[l] : 0.f;
    for (int l = n; l < ICPMI_MAX_VOXEL_LEVELS; ++l) { // a level the schedule no longer has gives its table back
        VoxLevel& lv = h->vox[l];
        (void)lv.keys.reset(); (void)lv.rec.reset(); (void)lv.tab.reset();
        lv.ready = false; lv.nv = 0;
    }
    h->vox_levels = n;
    h->voxel_size = n > 0 ? sizes[n - 1] : 0.f; // (no graph to drop: loop_sig hashes the level count and every level's size, generation and table; the tables follow lazily)
    h->vox_step_level = -1;
    for (int i = 0; i < 1 + 3 * ICPMI_MAX_VOXEL_LEVELS; ++i) h->vox_report[i] = 0;
}

icpmi_status icpmi_set_voxel_matcher(icpmi_handle h, float size)
{
    CHECK_H(h);
    if (!std::isfinite(size) || size < 0.f) { h->last_error = "set_voxel_matcher: the voxel size must be finite and >= 0 (0: off)"; return ICPMI_ERR_INVALID_ARG; }
    voxel_apply_schedule(h, &size, size > 0.f ? 1 : 0);
    return ICPMI_OK;
}

icpmi_status icpmi_get_voxel_matcher(icpmi_handle h, float* size)
{
    CHECK_H(h);
    if (!size) { h->last_error = "get_voxel_matcher: size is null"; return ICPMI_ERR_INVALID_ARG; }
    *size = h->voxel_size;
    return ICPMI_OK;
}

icpmi_status icpmi_set_voxel_schedule(icpmi_handle h, const float* sizes, int32_t n)
{
    CHECK_H(h);
    if (n < 0 || n > ICPMI_MAX_VOXEL_LEVELS || (n > 0 && !sizes)) {
        h->last_error = "InvalidParameter: set_voxel_schedule: VoxelMatcher takes 0 (off) to 4 voxel sizes"; return ICPMI_ERR_INVALID_ARG;
    }
    for (int l = 0; l < n; ++l) {
        if (!std::isfinite(sizes[l]) || !(sizes[l] > 0.f)) {
            h->last_error = "InvalidParameter: set_voxel_schedule: every voxel size of the VoxelMatcher schedule must be finite and > 0"; return ICPMI_ERR_INVALID_ARG;
        }
        if (l > 0 && !(sizes[l] < sizes[l - 1])) {
            h->last_error = "InvalidParameter: set_voxel_schedule: the voxel sizes of the VoxelMatcher schedule must be strictly descending (coarsest first)";
            return ICPMI_ERR_INVALID_ARG;
        }
    }
    voxel_apply_schedule(h, sizes, n);
    return ICPMI_OK;
}

icpmi_status icpmi_get_voxel_schedule(icpmi_handle h, float sizes[4], int32_t* n)
{
    CHECK_H(h);
    if (!sizes || !n) { h->last_error = "get_voxel_schedule: null argument"; return ICPMI_ERR_INVALID_ARG; }
    for (int l = 0; l < ICPMI_MAX_VOXEL_LEVELS; ++l) sizes[l] = h->vox_sizes[l];
    *n = h->vox_levels;
    return ICPMI_OK;
}

icpmi_status icpmi_get_voxel_schedule_report(icpmi_handle h, int32_t* levels, int32_t iterations[4], int32_t pairs_first[4], int32_t pairs_last[4])
{
    CHECK_H(h);
    if (!levels || !iterations || !pairs_first || !pairs_last) { h->last_error = "get_voxel_schedule_report: null argument"; return ICPMI_ERR_INVALID_ARG; }
    if (h->vox_levels < 2) { h->last_error = "get_voxel_schedule_report: the handle has no schedule of two or more voxel sizes (icpmi_set_voxel_schedule)"; return ICPMI_ERR_INVALID_ARG; }
    *levels = h->vox_report[0];
    for (int l = 0; l < ICPMI_MAX_VOXEL_LEVELS; ++l) {
        iterations[l] = h->vox_report[1 + l];
        pairs_first[l] = h->vox_report[1 + ICPMI_MAX_VOXEL_LEVELS + l];
        pairs_last[l] = h->vox_report[1 + 2 * ICPMI_MAX_VOXEL_LEVELS + l];
    }
    return ICPMI_OK;
}

// test seam: the level icpmi_minimize_step_normals evaluates on a scheduled handle (-1: the finest again); a new schedule resets it
icpmi_status icpmi_debug_voxel_step_level(icpmi_handle h, int32_t level)
{
    CHECK_H(h);
    if (level < -1 || level >= h->vox_levels) { h->last_error = "debug_voxel_step_level: no such level in the voxel schedule"; return ICPMI_ERR_INVALID_ARG; }
    h->vox_step_level = level;
    return ICPMI_OK;
}

static icpmi_status get_voxel_map_impl(icpmi_handle h, int level, int64_t cap, int32_t* ijk3, float* mean3, float* moments6, int32_t* count, int64_t* n_voxels)
{
    if (n_voxels) *n_voxels = 0;
    if (cap < 0) { h->last_error = "get_voxel_map: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return voxel_get_map(h, level, cap, ijk3, mean3, moments6, count, n_voxels);
}

icpmi_status icpmi_get_voxel_map(icpmi_handle h, int64_t cap, int32_t* ijk3, float* mean3, float* moments6, int32_t* count, int64_t* n_voxels)
{
    CHECK_H(h);
    return get_voxel_map_impl(h, -1, cap, ijk3, mean3, moments6, count, n_voxels);
}

icpmi_status icpmi_get_voxel_map_level(icpmi_handle h, int32_t level, int64_t cap, int32_t* ijk3, float* mean3, float* moments6, int32_t* count,
                                       int64_t* n_voxels)
{
    CHECK_H(h);
    if (level < 0) { if (n_voxels) *n_voxels = 0; h->last_error = "get_voxel_map_level: no such level in the voxel schedule"; return ICPMI_ERR_INVALID_ARG; }
    return get_voxel_map_impl(h, level, cap, ijk3, mean3, moments6, count, n_voxels);
}

icpmi_status icpmi_voxel_lookup(icpmi_handle h, const float* q4_centred, int64_t n, int32_t* voxel)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!q4_centred || !voxel))) { h->last_error = "voxel_lookup: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return voxel_lookup(h, -1, q4_centred, n, voxel);
}

icpmi_status icpmi_voxel_lookup_level(icpmi_handle h, int32_t level, const float* q4_centred, int64_t n, int32_t* voxel)
{
    CHECK_H(h);
    if (level < 0 || n < 0 || (n > 0 && (!q4_centred || !voxel))) { h->last_error = "voxel_lookup_level: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return voxel_lookup(h, level, q4_centred, n, voxel);
}

void icpmi_voxel_score_options_default(icpmi_voxel_score_options* opts)
{
    if (!opts) return;
    memset(opts, 0, sizeof *opts);
    opts->level = -1; opts->beta = 1.f;
}

void icpmi_voxel_score_shape(int32_t* slice, int32_t* tile)
{
    int32_t s = 0, t = 0;
    voxel_score_shape(&s, &t);
    if (slice) *slice = s;
    if (tile) *tile = t;
}

// icpmi_voxel_score_poses*: the whole call's checks, the table, then the rigid poses in the caller's order through voxel_score_poses
// (voxel.hip).  stage: the host variant's upload, run behind the checks and the table build
static icpmi_status voxel_score_impl(icpmi_handle h, const char* who, const float* scan4, bool on_host, int64_t n, const float* n3, const float* T,
                                     int32_t n_poses, const icpmi_voxel_score_options* opts, icpmi_voxel_score* out, icpmi_status* status)
{
    h->read_scalar_n = 0; h->read_noise_n = 0; h->read_r2_n = 0; h->read_int_n = 0; // (the one-shot reading rows belong to this call)
    // zeroed on every whole-call error; a count above the limit zeroes the limit's worth: a wild n_poses must not size a write
    const size_t n_zero = n_poses < 1 ? 0 : (size_t)(n_poses > 4096 ? 4096 : n_poses);
    if (out && n_zero) memset(out, 0, sizeof(icpmi_voxel_score) * n_zero);
    if (status && n_zero) memset(status, 0, sizeof(icpmi_status) * n_zero);
    if (!voxel_path(h)) {
        h->last_error = std::string(who) + ": the handle is not on the voxel path (icpmi_set_voxel_matcher > 0 on PlaneToPlaneErrorMinimizer with the GICP pair model)";
        return ICPMI_ERR_UNSUPPORTED;
    }
    icpmi_voxel_score_options o;
    icpmi_voxel_score_options_default(&o);
    if (opts) o = *opts;
    if (!out || !T || n_poses < 1 || n_poses > 4096 || n < 0 || (n > 0 && !scan4)) {
        h->last_error = std::string(who) + ": bad arguments (1 <= n_poses <= 4096)"; return ICPMI_ERR_INVALID_ARG;
    }
    if (!std::isfinite(o.beta) || !(o.beta > 0.f)) { h->last_error = std::string(who) + ": beta must be finite and > 0"; return ICPMI_ERR_INVALID_ARG; }
    if (h->m <= 0) { h->last_error = std::string(who) + ": no map"; return ICPMI_ERR_INVALID_ARG; }
    int level = o.level;
    if (level == -1) level = h->vox_levels - 1;
    if (level < 0 || level >= h->vox_levels) { h->last_error = std::string(who) + ": no such level in the voxel schedule"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffff / ICPMI_MAX_K) { h->last_error = std::string(who) + ": too many points"; return ICPMI_ERR_UNSUPPORTED; }
    if (!h->has_normals) { h->last_error = "InvalidField: VoxelMatcher needs the descriptor 'normals' on the map"; return ICPMI_ERR_MISSING_NORMALS; }
    if (!n3) { h->last_error = std::string(who) + ": the voxel score needs the reading's normals"; return ICPMI_ERR_MISSING_NORMALS; }
    if (n == 0) { h->last_error = std::string(who) + ": the reading is empty"; return ICPMI_ERR_NO_POINT_TO_MINIMIZE; }
    { const icpmi_status ts = voxel_ensure_table(h, nullptr); if (ts != ICPMI_OK) return ts; }
    const float* d_scan = scan4;
    const float* d_n3 = n3;
    if (on_host) { const icpmi_status ss = stage_in_scratch(h, scan4, n, n3, &d_scan, &d_n3); if (ss != ICPMI_OK) return ss; }
    const float hb = 0.5f * o.beta;
    std::vector<icpmi_status> st((size_t)n_poses, ICPMI_OK);
    std::vector<int> live;
    std::vector<float> Tc;
    for (int p = 0; p < n_poses; ++p) {
        st[(size_t)p] = check_rigid(h, T + 16 * (size_t)p);
        if (st[(size_t)p] != ICPMI_OK) continue;
        live.push_back(p);
        Tc.resize(Tc.size() + 16);
        centred_pose(h, T + 16 * (size_t)p, Tc.data() + Tc.size() - 16);
    }
    if (!live.empty()) {
        std::vector<icpmi_voxel_score> ro(live.size());
        const icpmi_status vs = voxel_score_poses(h, (const float4*)d_scan, n, d_n3, Tc.data(), (int)live.size(), level, hb, ro.data());
        if (vs != ICPMI_OK) { memset(out, 0, sizeof(icpmi_voxel_score) * (size_t)n_poses); return vs; }
        for (size_t i = 0; i < live.size(); ++i) {
            out[live[i]] = ro[i];
            if (ro[i].pairs == 0) st[(size_t)live[i]] = ICPMI_ERR_NO_POINT_TO_MINIMIZE;
        }
    }
    return fold_status(h, status, st.data(), n_poses, (std::string(who) + ": a pose ended with an error (see the per-pose status)").c_str());
}

icpmi_status icpmi_voxel_score_poses_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_scan_normals3, const float* T,
                                         int32_t n_poses, const icpmi_voxel_score_options* opts, icpmi_voxel_score* out, icpmi_status* status)
{
    CHECK_H(h);
    return voxel_score_impl(h, "voxel_score_poses_dev", d_scan4, false, n, d_scan_normals3, T, n_poses, opts, out, status);
}

icpmi_status icpmi_voxel_score_poses(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float* T, int32_t n_poses,
                                     const icpmi_voxel_score_options* opts, icpmi_voxel_score* out, icpmi_status* status)
{
    CHECK_H(h);
    return voxel_score_impl(h, "voxel_score_poses", scan4, true, n, scan_normals3, T, n_poses, opts, out, status);
}

// ---- global localisation (occupancy.hip) ----
void icpmi_global_localize_options_default(icpmi_global_localize_options* opts)
{
    if (!opts) return;
    memset(opts, 0, sizeof *opts);
    opts->cell_size = 0.5f; opts->batch = 64;
}

void icpmi_global_localize_shape(int32_t* slice, int32_t* tile, int32_t* launch_nodes)
{
    int32_t s = 0, t = 0, ln = 0;
    occ_shape(&s, &t, &ln);
    if (slice) *slice = s;
    if (tile) *tile = t;
    if (launch_nodes) *launch_nodes = ln;
}

// what the occupancy calls share: a map, no planar mode, a reading, rigid rotations, a cell size, a level count in [lmin, 8]
static icpmi_status occupancy_checks(icpmi_handle h, const char* who, const float* scan4, int64_t n, const float* R9, int32_t n_rot, float s0, int32_t levels,
                                     int32_t lmin)
{
    const std::string w(who);
    if (h->cfg.force_2d || h->cfg.is_2d) { h->last_error = w + ": is not served in planar mode (force_2d / is_2d)"; return ICPMI_ERR_UNSUPPORTED; }
    if (h->m <= 0) { h->last_error = w + ": no map"; return ICPMI_ERR_INVALID_ARG; }
    if (n_rot < 1 || n_rot > 4096) { h->last_error = w + ": n_rot must be in 1 .. 4096"; return ICPMI_ERR_INVALID_ARG; }
    if (!R9 || n < 0 || (n > 0 && !scan4)) { h->last_error = w + ": bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (!std::isfinite(s0) || !(s0 > 0.f)) { h->last_error = w + ": the cell size must be finite and > 0"; return ICPMI_ERR_INVALID_ARG; }
    if (levels < lmin || levels > ICPMI_MAX_OCC_LEVELS) { h->last_error = w + ": levels must be in " + (lmin ? "1" : "0") + " .. 8"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffff) { h->last_error = w + ": too many points"; return ICPMI_ERR_UNSUPPORTED; }
    for (int k = 0; k < n_rot; ++k) {
        float T[16] = {0};
        for (int cc = 0; cc < 3; ++cc) for (int r = 0; r < 3; ++r) T[4 * cc + r] = R9[9 * (size_t)k + 3 * cc + r];
        T[15] = 1.f;
        bool finite = true;
        for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(R9[9 * (size_t)k + i]);
        if (!finite || check_rigid(h, T) != ICPMI_OK) {
            h->last_error = w + ": rotation " + std::to_string(k) + ": TransformationError: RigidTransformation: rotation part is not orthonormal (|1 - det| > 1e-3)";
            return ICPMI_ERR_INVALID_ARG;
        }
    }
    if (n == 0) { h->last_error = w + ": the reading is empty"; return ICPMI_ERR_NO_POINT_TO_MINIMIZE; }
    return ICPMI_OK;
}

static icpmi_status global_localize_impl(icpmi_handle h, const char* who, const float* scan4, bool on_host, int64_t n, const float* R9, int32_t n_rot,
                                         const icpmi_global_localize_options* opts, icpmi_global_localize_result* res)
{
    const std::string w(who);
    if (!res) { h->last_error = w + ": result is null"; return ICPMI_ERR_INVALID_ARG; }
    memset(res, 0, sizeof *res);
    res->rotation = -1;
    res->T[0] = res->T[5] = res->T[10] = res->T[15] = 1.f;
    icpmi_global_localize_options o;
    icpmi_global_localize_options_default(&o);
    if (opts) o = *opts;
    { const icpmi_status s = occupancy_checks(h, who, scan4, n, R9, n_rot, o.cell_size, o.levels, 0); if (s != ICPMI_OK) return s; }
    if (o.batch < 1 || o.batch > 8192) { h->last_error = w + ": batch must be in 1 .. 8192"; return ICPMI_ERR_INVALID_ARG; }
    if (o.max_nodes < 0) { h->last_error = w + ": max_nodes must be >= 0"; return ICPMI_ERR_INVALID_ARG; }
    if (!std::isfinite(o.min_score_ratio) || o.min_score_ratio < 0.f || o.min_score_ratio > 1.f) {
        h->last_error = w + ": min_score_ratio must be in 0 .. 1"; return ICPMI_ERR_INVALID_ARG;
    }
    int64_t a_min[3] = {0, 0, 0}, a_max[3] = {0, 0, 0};
    if (o.has_box) {
        for (int j = 0; j < 3; ++j) {
            const double lo = o.box_lo[j], hi = o.box_hi[j];
            const double fl = floor((lo - (double)h->mean[j]) / (double)o.cell_size), fh = floor((hi - (double)h->mean[j]) / (double)o.cell_size);
            if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi) || !(fabs(fl) < 524288.0) || !(fabs(fh) < 524288.0)) {
                h->last_error = w + ": bad box (finite, lo <= hi, within 2^19 cells of the map's centroid)"; return ICPMI_ERR_INVALID_ARG;
            }
            a_min[j] = (int64_t)fl; a_max[j] = (int64_t)fh;
        }
    }
    // the window's extent decides an automatic level count; without a box the window is the extent of the pyramid's level 0
    int levels = o.levels;
    if (!o.has_box) {
        { const icpmi_status s = occ_ensure(h, o.cell_size, levels ? levels : 1); if (s != ICPMI_OK) return s; }
        for (int j = 0; j < 3; ++j) { a_min[j] = h->occ.cell_lo[j]; a_max[j] = h->occ.cell_hi[j]; }
    }
    if (levels == 0) {
        int64_t side = 1;
        for (int j = 0; j < 3; ++j) side = std::max<int64_t>(side, a_max[j] - a_min[j] + 1);
        levels = 1;
        while (levels < 6 && ((int64_t)1 << levels) <= side) ++levels;
    }
    const float* d_scan = scan4;
    if (on_host) { const float* none = nullptr; const icpmi_status ss = stage_in_scratch(h, scan4, n, nullptr, &d_scan, &none); if (ss != ICPMI_OK) return ss; }
    const int64_t need = (int64_t)ceil((double)o.min_score_ratio * (double)n);
    const icpmi_status s = occ_global_localize(h, (const float4*)d_scan, n, R9, n_rot, o.cell_size, levels, a_min, a_max, o.batch, need, o.max_nodes, res);
    if (s != ICPMI_OK) { memset(res, 0, sizeof *res); res->rotation = -1; res->T[0] = res->T[5] = res->T[10] = res->T[15] = 1.f; }
    return s;
}

icpmi_status icpmi_global_localize(icpmi_handle h, const float* scan4, int64_t n, const float* R9, int32_t n_rot, const icpmi_global_localize_options* opts,
                                   icpmi_global_localize_result* result)
{
    CHECK_H(h);
    return global_localize_impl(h, "global_localize", scan4, true, n, R9, n_rot, opts, result);
}

icpmi_status icpmi_global_localize_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* R9, int32_t n_rot,
                                       const icpmi_global_localize_options* opts, icpmi_global_localize_result* result)
{
    CHECK_H(h);
    return global_localize_impl(h, "global_localize_dev", d_scan4, false, n, R9, n_rot, opts, result);
}

icpmi_status icpmi_occupancy_score_nodes(icpmi_handle h, const float* scan4, int64_t n, const float* R9, int32_t n_rot, float s0, int32_t levels,
                                         const int32_t* nodes5, int64_t n_nodes, int64_t* counts)
{
    CHECK_H(h);
    { const icpmi_status s = occupancy_checks(h, "occupancy_score_nodes", scan4, n, R9, n_rot, s0, levels, 1); if (s != ICPMI_OK) return s; }
    if (n_nodes < 0 || (n_nodes > 0 && (!nodes5 || !counts))) { h->last_error = "occupancy_score_nodes: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    for (int64_t q = 0; q < n_nodes; ++q) {
        const int32_t* f = nodes5 + 5 * q;
        bool ok = f[0] >= 0 && f[0] < n_rot && f[1] >= 0 && f[1] < levels;
        for (int j = 0; j < 3; ++j) ok = ok && f[2 + j] > -524288 && f[2 + j] < 524288;
        if (!ok) { h->last_error = "occupancy_score_nodes: node " + std::to_string(q) + " is not (k in [0, n_rot), l in [0, levels), |A| < 2^19)"; return ICPMI_ERR_INVALID_ARG; }
    }
    if (n_nodes == 0) return ICPMI_OK;
    const float* d_scan = nullptr; const float* none = nullptr;
    { const icpmi_status ss = stage_in_scratch(h, scan4, n, nullptr, &d_scan, &none); if (ss != ICPMI_OK) return ss; }
    return occ_score_nodes(h, (const float4*)d_scan, n, R9, n_rot, s0, levels, nodes5, n_nodes, counts);
}

icpmi_status icpmi_get_occupancy_level(icpmi_handle h, float s0, int32_t levels, int32_t level, int64_t cap, int32_t* ijk3, int64_t* n_keys)
{
    CHECK_H(h);
    if (n_keys) *n_keys = 0;
    if (h->cfg.force_2d || h->cfg.is_2d) { h->last_error = "get_occupancy_level: is not served in planar mode (force_2d / is_2d)"; return ICPMI_ERR_UNSUPPORTED; }
    if (h->m <= 0) { h->last_error = "get_occupancy_level: no map"; return ICPMI_ERR_INVALID_ARG; }
    if (!std::isfinite(s0) || !(s0 > 0.f) || levels < 1 || levels > ICPMI_MAX_OCC_LEVELS || level < 0 || level >= levels || cap < 0) {
        h->last_error = "get_occupancy_level: bad arguments (a finite cell size > 0, levels in 1 .. 8, level in [0, levels))"; return ICPMI_ERR_INVALID_ARG;
    }
    return occ_get_level(h, s0, levels, level, cap, ijk3, n_keys);
}

icpmi_status icpmi_get_occupancy_info(icpmi_handle h, int32_t* levels, int64_t keys[8], int64_t bytes[8], float build_ms[8], int64_t* builds)
{
    CHECK_H(h);
    const OccPyramid& p = h->occ;
    const int L = p.ready ? p.levels : 0;
    if (levels) *levels = L;
    if (builds) *builds = (int64_t)p.builds;
    for (int l = 0; l < ICPMI_MAX_OCC_LEVELS; ++l) {
        const bool on = l < L;
        if (keys) keys[l] = on ? p.lv[l].nk : 0;
        if (bytes) bytes[l] = on ? (int64_t)(sizeof(unsigned long long) * ((size_t)p.lv[l].nk + (size_t)p.lv[l].mask + 1)) : 0;
        if (build_ms) build_ms[l] = on ? p.lv[l].build_ms : 0.f;
    }
    return ICPMI_OK;
}

// test seam of scripts/voxel_bench.py: rebuilds the table and reports what its three stages took (sort, reduce, fill; milliseconds by HIP events)
icpmi_status icpmi_debug_voxel_build_times(icpmi_handle h, float times_ms3[3])
{
    CHECK_H(h);
    if (!times_ms3) { h->last_error = "debug_voxel_build_times: times is null"; return ICPMI_ERR_INVALID_ARG; }
    return voxel_ensure_table(h, times_ms3);
}

// ... and what one lookup launch of n queries takes through the table (ms2[0]) and by binary search over the sorted keys (ms2[1])
icpmi_status icpmi_debug_voxel_lookup_times(icpmi_handle h, const float* q4_centred, int64_t n, int32_t reps, float ms2[2], int64_t* mismatch)
{
    CHECK_H(h);
    if (!q4_centred || n < 1 || reps < 1 || !ms2) { h->last_error = "debug_voxel_lookup_times: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return voxel_lookup_times(h, q4_centred, n, reps, ms2, mismatch);
}

icpmi_status icpmi_set_intensity_weight(icpmi_handle h, float w)
{
    CHECK_H(h);
    if (!std::isfinite(w) || !(w >= 0.f) || !(w < 1.f)) { h->last_error = "set_intensity_weight: the weight (1 - lambdaGeometric) must be finite and in [0, 1)"; return ICPMI_ERR_INVALID_ARG; }
    h->intensity_w = w; // (no graph to drop: make_loop_cfg puts it into the LoopCfg, which loop_sig hashes)
    return ICPMI_OK;
}

icpmi_status icpmi_get_intensity_weight(icpmi_handle h, float* w)
{
    CHECK_H(h);
    if (!w) { h->last_error = "get_intensity_weight: w is null"; return ICPMI_ERR_INVALID_ARG; }
    *w = h->intensity_w;
    return ICPMI_OK;
}

icpmi_status icpmi_set_map_intensity(icpmi_handle h, const float* intensity, int64_t m, int32_t knn)
{
    CHECK_H(h);
    h->gi_m = 0; // (a failed call leaves no channel)
    if (!intensity || m <= 0 || m != h->m) { h->last_error = "set_map_intensity: one intensity per point of the resident map (m must equal its size)"; return ICPMI_ERR_INVALID_ARG; }
    if (!h->has_normals) { h->last_error = "InvalidField: set_map_intensity needs the descriptor 'normals' on the map (the gradients live in its tangent planes)"; return ICPMI_ERR_MISSING_NORMALS; }
    return ops_set_map_intensity(h, intensity, m, knn);
}

icpmi_status icpmi_intensity_gradient(icpmi_handle h, const float* pts4, int64_t m, const float* normals3, const float* intensity, int32_t knn,
                                      float* grad3_out)
{
    CHECK_H(h);
    if (m < 0 || (m > 0 && (!pts4 || !normals3 || !intensity || !grad3_out))) { h->last_error = "intensity_gradient: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_intensity_gradient(h, pts4, m, normals3, intensity, knn, grad3_out);
}

icpmi_status icpmi_surface_normals(icpmi_handle h, const float* pts4, int64_t m, int32_t knn, float* normals3)
{
    CHECK_H(h);
    if (m < 0 || (m > 0 && (!pts4 || !normals3))) { h->last_error = "surface_normals: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_surface_normals(h, pts4, m, knn, normals3);
}

icpmi_status icpmi_surface_normals_ex(icpmi_handle h, const float* pts4, int64_t m, int32_t knn, float* normals3, float* densities)
{
    CHECK_H(h);
    if (m < 0 || (m > 0 && (!pts4 || !normals3))) { h->last_error = "surface_normals: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_surface_normals(h, pts4, m, knn, normals3, densities);
}

icpmi_status icpmi_surface_normals_ex2(icpmi_handle h, const float* pts4, int64_t m, int32_t knn, float* normals3, float* densities,
                                       int32_t* matched_ids, float* mean_dist)
{
    CHECK_H(h);
    if (m < 0 || (m > 0 && (!pts4 || !normals3))) { h->last_error = "surface_normals: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_surface_normals(h, pts4, m, knn, normals3, densities, matched_ids, mean_dist);
}

icpmi_status icpmi_surface_normals_ex3(icpmi_handle h, const float* pts4, int64_t m, int32_t knn, float* normals3, float* densities,
                                       int32_t* matched_ids, float* mean_dist, float* eig_values3, float* eig_vectors9)
{
    CHECK_H(h);
    if (m < 0 || (m > 0 && (!pts4 || !normals3))) { h->last_error = "surface_normals: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_surface_normals(h, pts4, m, knn, normals3, densities, matched_ids, mean_dist, eig_values3, eig_vectors9);
}

icpmi_status icpmi_point_distance_keep(icpmi_handle h, const float* map4, int64_t m, const float* in4, int64_t n, float min_dist,
                                       uint8_t* keep)
{
    CHECK_H(h);
    if (m < 0 || n < 0 || (m > 0 && !map4) || (n > 0 && (!in4 || !keep))) { h->last_error = "point_distance_keep: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_point_distance_keep(h, map4, m, in4, n, min_dist, keep);
}

icpmi_status icpmi_map_update_point_distance(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, float min_dist,
                                             int32_t normals_knn, uint8_t* keep_out, int64_t* appended, int64_t* new_m)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !scan4) || !(min_dist >= 0.f)) { h->last_error = "map_update_point_distance: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_map_update_point_distance(h, scan4, n, scan_normals3, min_dist, normals_knn, keep_out, appended, new_m);
}

icpmi_status icpmi_register_prior(icpmi_handle h, const float* scan4, int64_t n, const float prior[16], float T_out[16], icpmi_stats* stats)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !scan4) || !prior) { h->last_error = "register_prior: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    h->scan_map_n = 0;
    if (n > 0) {
        if (h->d_stage_in.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        if (h->d_scan_map.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        HIP_TRY(h, hipMemcpyAsync(h->d_stage_in, scan4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
        icpmi_status s = ops_transform_dev(h, prior, h->d_stage_in, n, h->d_scan_map); // Mapper.cpp:197
        if (s != ICPMI_OK) return s;
        h->scan_map_n = n;
    }
    return register_impl(h, (const float*)h->d_scan_map.get(), n, nullptr, 0, T_out, stats);
}

// ... with the scan already in HBM (sensor frame): what a scan stream that lives on the device -- or a benchmark that must not time
// PCIe -- hands over; everything else as icpmi_register_prior
icpmi_status icpmi_register_prior_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float prior[16], float T_out[16], icpmi_stats* stats)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !d_scan4) || !prior) { h->last_error = "register_prior_dev: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    h->scan_map_n = 0;
    if (n > 0) {
        if (h->d_scan_map.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        icpmi_status s = ops_transform_dev(h, prior, (const float4*)d_scan4, n, h->d_scan_map); // Mapper.cpp:197
        if (s != ICPMI_OK) return s;
        h->scan_map_n = n;
    }
    return register_impl(h, (const float*)h->d_scan_map.get(), n, nullptr, 0, T_out, stats);
}

icpmi_status icpmi_map_update_staged(icpmi_handle h, const float correction[16], float min_dist, int32_t normals_knn, uint8_t* keep_out,
                                     int64_t* appended, int64_t* new_m)
{
    CHECK_H(h);
    if (!correction || !(min_dist >= 0.f)) { h->last_error = "map_update_staged: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (h->scan_map_n <= 0) { h->last_error = "map_update_staged: no scan staged by icpmi_register_prior"; return ICPMI_ERR_INVALID_ARG; }
    const int64_t n = h->scan_map_n;
    if (h->d_stage_in.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    icpmi_status s = ops_transform_dev(h, correction, h->d_scan_map, n, h->d_stage_in); // Mapper.cpp:221
    if (s != ICPMI_OK) return s;
    return ops_map_update_dev(h, h->d_stage_in, n, nullptr, min_dist, normals_knn, keep_out, appended, new_m);
}

icpmi_status icpmi_staged_point_distance_keep(icpmi_handle h, const float correction[16], float min_dist, uint8_t* keep_out, float* placed_out4)
{
    CHECK_H(h);
    if (!correction || !keep_out || !(min_dist >= 0.f)) { h->last_error = "staged_point_distance_keep: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (h->scan_map_n <= 0) { h->last_error = "staged_point_distance_keep: no scan staged by icpmi_register_prior"; return ICPMI_ERR_INVALID_ARG; }
    return ops_staged_keep(h, correction, min_dist, keep_out, placed_out4);
}

icpmi_status icpmi_comm_get_unique_id(icpmi_comm_id* id)
{
    if (!id) { g_create_error = "comm_get_unique_id: null argument"; return ICPMI_ERR_INVALID_ARG; }
    return comm_unique_id(id, g_create_error);
}

icpmi_status icpmi_comm_init(icpmi_handle h, const icpmi_comm_id* id, int32_t n_ranks, int32_t rank)
{
    CHECK_H(h);
    if (!id || n_ranks < 1 || rank < 0 || rank >= n_ranks) { h->last_error = "comm_init: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return comm_init(h, id, n_ranks, rank);
}

icpmi_status icpmi_comm_info(icpmi_handle h, int32_t* n_ranks, int32_t* rank, int32_t* kind)
{
    CHECK_H(h);
    int a = 1, b = 0, k = 0;
    const icpmi_status s = comm_info(h, &a, &b, &k);
    if (n_ranks) *n_ranks = a;
    if (rank) *rank = b;
    if (kind) *kind = k;
    return s;
}

icpmi_status icpmi_comm_destroy(icpmi_handle h)
{
    CHECK_H(h);
    return comm_destroy(h);
}

icpmi_status icpmi_staged_merge_allgather(icpmi_handle h, const float correction[16], float min_dist, int32_t normals_knn,
                                          int64_t* accepted_local, int64_t* appended_total, int64_t* new_m, float* merged_out4,
                                          int64_t merged_capacity, int64_t* merged_n)
{
    CHECK_H(h);
    // (argument errors are local by construction: every rank passes the same min_dist / normals_knn, and a rank that hands in
    // garbage here has a bug no protocol can paper over)
    if (!(min_dist >= 0.f) || normals_knn < 0 || normals_knn > ICPMI_MAX_K || merged_capacity < 0) {
        h->last_error = "staged_merge_allgather: bad arguments"; return ICPMI_ERR_INVALID_ARG;
    }
    // correction == NULL or nothing staged: this rank contributes no points and still takes part in the exchange
    return ops_staged_merge_allgather(h, correction, min_dist, normals_knn, accepted_local, appended_total, new_m, merged_out4, merged_capacity, merged_n);
}

icpmi_status icpmi_staged_merged_points(icpmi_handle h, float* out4, int64_t capacity, int64_t* n)
{
    CHECK_H(h);
    if (capacity < 0) { h->last_error = "staged_merged_points: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_staged_merged_points(h, out4, capacity, n);
}

icpmi_status icpmi_staged_bin_cells(icpmi_handle h, float cell_size, int32_t* ijk3, int64_t* offsets, int64_t* counts, int64_t capacity, int64_t* n_cells)
{
    CHECK_H(h);
    if (!(cell_size > 0.f) || capacity < 0) { h->last_error = "staged_bin_cells: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_staged_bin_cells(h, cell_size, ijk3, offsets, counts, capacity, n_cells);
}

icpmi_status icpmi_cell_log_configure(icpmi_handle h, float cell_size)
{
    CHECK_H(h);
    if (!(cell_size >= 0.f)) { h->last_error = "cell_log_configure: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    h->cell_auto_size = cell_size;
    return ICPMI_OK;
}

icpmi_status icpmi_cell_log_read(icpmi_handle h, int64_t offset, int64_t count, float* out4, int64_t* log_size)
{
    CHECK_H(h);
    return ops_cell_log_read(h, offset, count, out4, log_size);
}

icpmi_status icpmi_cell_log_clear(icpmi_handle h)
{
    CHECK_H(h);
    return ops_cell_log_clear(h);
}

icpmi_status icpmi_stage_discard(icpmi_handle h)
{
    CHECK_H(h);
    h->scan_map_n = 0;
    return ICPMI_OK;
}

icpmi_status icpmi_get_map(icpmi_handle h, float* out4, float* normals3, int64_t capacity, int64_t* m)
{
    CHECK_H(h);
    return ops_get_map(h, out4, normals3, capacity, m);
}

icpmi_status icpmi_voxel_keep(icpmi_handle h, const float* in4, int64_t n, float edge, int32_t method, uint8_t* keep)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!in4 || !keep)) || !(edge > 0.f) || (method != 0 && method != 1)) { h->last_error = "voxel_keep: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_voxel_keep_first(h, in4, n, edge, method, keep);
}

icpmi_status icpmi_sampling_surface_normal(icpmi_handle h, const float* in4, int64_t n, float ratio, int32_t knn, float max_box_dim, int32_t seed,
                                           int32_t* order_out, float* normals3_out, int64_t* n_out)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !in4) || !(ratio > 0.f) || !(ratio <= 1.f) || knn < 3 || !(max_box_dim > 0.f) || seed < 0) {
        h->last_error = "sampling_surface_normal: bad arguments (0 < ratio <= 1, knn >= 3, maxBoxDim > 0, seed >= 0)"; return ICPMI_ERR_INVALID_ARG;
    }
    return ops_sampling_surface_normal(h, in4, n, ratio, knn, max_box_dim, seed, order_out, normals3_out, n_out);
}

icpmi_status icpmi_sampling_surface_normal_ex(icpmi_handle h, const float* in4, int64_t n, float ratio, int32_t knn, float max_box_dim, int32_t seed,
                                              int32_t method, int32_t* order_out, float* normals3_out, int64_t* n_out, float* mean3_out,
                                              int32_t* member_start_out, int32_t* member_count_out, int32_t* members_out)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !in4) || !(ratio > 0.f) || !(ratio <= 1.f) || knn < 3 || !(max_box_dim > 0.f) || seed < 0 || (method != 0 && method != 1)) {
        h->last_error = "sampling_surface_normal: bad arguments (0 < ratio <= 1, knn >= 3, maxBoxDim > 0, seed >= 0, samplingMethod 0 or 1)"; return ICPMI_ERR_INVALID_ARG;
    }
    return ops_sampling_surface_normal_ex(h, in4, n, ratio, knn, max_box_dim, seed, method, order_out, normals3_out, n_out, mean3_out, member_start_out,
                                          member_count_out, members_out);
}

icpmi_status icpmi_octree_sample(icpmi_handle h, const float* in4, int64_t n, float max_size, int32_t max_points, int32_t method,
                                 int32_t* order_out, int32_t* leaf_of_out, int64_t* n_out)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !in4) || !(max_size >= 0.f) || max_points < 0 || (method != 0 && method != 1)) { h->last_error = "octree_sample: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_octree_sample(h, in4, n, max_size, max_points, method, order_out, leaf_of_out, n_out);
}

icpmi_status icpmi_voxel_grid(icpmi_handle h, const float* in4, int64_t n, const float vsize[3], int32_t average_descriptors, const float* desc,
                              int32_t desc_rows, int32_t* order_out, float* out4, float* desc_out, int64_t* n_out)
{
    CHECK_H(h);
    if (n_out) *n_out = 0;
    if (n < 0 || !n_out || (n > 0 && (!in4 || !out4)) || !vsize || desc_rows < 0 || (desc_rows > 0 && n > 0 && (!desc || !desc_out)) ||
        (average_descriptors != 0 && average_descriptors != 1)) {
        h->last_error = "voxel_grid: bad arguments"; return ICPMI_ERR_INVALID_ARG;
    }
    for (int r = 0; r < 3; ++r)
        if (!(vsize[r] > 0.f) || !std::isfinite(vsize[r])) { h->last_error = "voxel_grid: vSizeX / vSizeY / vSizeZ must be finite and > 0"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffffll) { h->last_error = "voxel_grid: more than 2^31 - 1 points"; return ICPMI_ERR_UNSUPPORTED; }
    return ops_voxel_grid(h, in4, n, vsize, average_descriptors, desc_rows > 0 ? desc : nullptr, desc_rows, order_out, out4, desc_out, n_out);
}

icpmi_status icpmi_covariance_sampling(icpmi_handle h, const float* in4, int64_t n, const float* normals3, int64_t nb_sample, int32_t torque_norm,
                                       int32_t* order_out, int64_t* n_out, icpmi_covsamp_info* info_out)
{
    CHECK_H(h);
    if (n_out) *n_out = 0;
    if (n < 0 || !n_out || (n > 0 && (!in4 || (nb_sample > 0 && !order_out)))) { h->last_error = "covariance_sampling: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (nb_sample < 0) { h->last_error = "covariance_sampling: nbSample must be >= 0"; return ICPMI_ERR_INVALID_ARG; }
    if (torque_norm < 0 || torque_norm > 2) { h->last_error = "covariance_sampling: torqueNorm must be 0 (L1), 1 (Lavg) or 2 (Lmax)"; return ICPMI_ERR_INVALID_ARG; }
    if (h->cfg.is_2d) { h->last_error = "covariance_sampling: planar (2-D) clouds are not supported (upstream takes 3-D clouds only)"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffffll) { h->last_error = "covariance_sampling: more than 2^31 - 1 points"; return ICPMI_ERR_UNSUPPORTED; }
    if (nb_sample >= n) {
        for (int64_t i = 0; i < n; ++i) order_out[i] = (int32_t)i;
        *n_out = n;
        return ICPMI_OK;
    }
    if (!normals3) { h->last_error = "covariance_sampling: the cloud has no normals (InvalidField normals)"; return ICPMI_ERR_MISSING_NORMALS; }
    const icpmi_status s = ops_covariance_sampling(h, in4, n, normals3, nb_sample, torque_norm, order_out, info_out);
    if (s == ICPMI_OK) *n_out = nb_sample;
    return s;
}

icpmi_status icpmi_normal_space_sampling(icpmi_handle h, const float* in4, int64_t n, const float* normals3, int64_t nb_sample, int32_t seed, float epsilon,
                                         int32_t* order_out, int64_t* n_out, int32_t* bucket_out)
{
    CHECK_H(h);
    if (n_out) *n_out = 0;
    if (n < 0 || !n_out || (n > 0 && (!in4 || (nb_sample > 0 && !order_out)))) { h->last_error = "normal_space_sampling: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (nb_sample < 0) { h->last_error = "normal_space_sampling: nbSample must be >= 0"; return ICPMI_ERR_INVALID_ARG; }
    if (seed < 0) { h->last_error = "normal_space_sampling: seed must be in [0, 2147483647]"; return ICPMI_ERR_INVALID_ARG; }
    if (!(epsilon >= 0.04908f && epsilon <= 3.14159f)) { h->last_error = "normal_space_sampling: epsilon must be in [0.04908, 3.14159]"; return ICPMI_ERR_INVALID_ARG; }
    if (h->cfg.is_2d) { h->last_error = "normal_space_sampling: planar (2-D) clouds are not supported (upstream takes 3-D clouds only)"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffffll) { h->last_error = "normal_space_sampling: more than 2^31 - 1 points"; return ICPMI_ERR_UNSUPPORTED; }
    if (nb_sample >= n) {
        for (int64_t i = 0; i < n; ++i) order_out[i] = (int32_t)i;
        *n_out = n;
        return ICPMI_OK;
    }
    if (!normals3) { h->last_error = "normal_space_sampling: the cloud has no normals (InvalidField normals)"; return ICPMI_ERR_MISSING_NORMALS; }
    if (nb_sample == 0) return ICPMI_OK;
    const icpmi_status s = ops_normal_space_sampling(h, in4, n, normals3, nb_sample, (unsigned)seed, epsilon, order_out, bucket_out);
    if (s == ICPMI_OK) *n_out = nb_sample;
    return s;
}

icpmi_status icpmi_voxel_keep_first(icpmi_handle h, const float* in4, int64_t n, float edge, uint8_t* keep)
{
    return icpmi_voxel_keep(h, in4, n, edge, 0, keep);
}

static icpmi_status stage_chain_scalar(icpmi_handle h, const float* scan_scalar, int64_t n)
{
    if (!scan_scalar || n == 0) return ICPMI_OK;
    if (h->d_stage_s.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(h->d_stage_s, scan_scalar, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    return ICPMI_OK;
}

static bool chain_needs_pose(const icpmi_map_op* ops, int32_t n_ops)
{
    for (int32_t i = 0; ops && i < n_ops; ++i) if (ops[i].type == ICPMI_MOP_DYNAMIC_POINTS) return true;
    return false;
}

icpmi_status icpmi_map_update_chain(icpmi_handle h, const float* scan4, int64_t n, const float* scan_normals3, const float* scan_scalar,
                                    const float to_sensor[16], const float from_sensor[16], const icpmi_map_op* ops, int32_t n_ops,
                                    int32_t n_modules, int32_t* src_out, int64_t src_capacity, int64_t* identity_prefix, int64_t* new_m)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && !scan4) || (chain_needs_pose(ops, n_ops) && !to_sensor) || (from_sensor && !to_sensor)) { h->last_error = "map_update_chain: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0) {
        if (h->d_stage_in.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        HIP_TRY(h, hipMemcpyAsync(h->d_stage_in, scan4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
        if (scan_normals3) {
            if (h->d_stage_n3.ensure(h, (size_t)n * 3) != ICPMI_OK) return ICPMI_ERR_HIP;
            HIP_TRY(h, hipMemcpyAsync(h->d_stage_n3, scan_normals3, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        }
        icpmi_status s = stage_chain_scalar(h, scan_scalar, n);
        if (s != ICPMI_OK) return s;
    }
    return ops_map_update_chain(h, h->d_stage_in, n, scan_normals3 ? h->d_stage_n3 : nullptr, scan_scalar ? h->d_stage_s : nullptr, to_sensor,
                                from_sensor, ops, n_ops, n_modules, src_out, src_capacity, identity_prefix, new_m);
}

icpmi_status icpmi_map_update_chain_staged(icpmi_handle h, const float correction[16], const float* scan_scalar, const float to_sensor[16],
                                           const float from_sensor[16], const icpmi_map_op* ops, int32_t n_ops, int32_t n_modules,
                                           int32_t* src_out, int64_t src_capacity, int64_t* identity_prefix, int64_t* new_m)
{
    CHECK_H(h);
    if (!correction || (chain_needs_pose(ops, n_ops) && !to_sensor) || (from_sensor && !to_sensor)) { h->last_error = "map_update_chain_staged: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (h->scan_map_n <= 0) { h->last_error = "map_update_chain_staged: no scan staged by icpmi_register_prior"; return ICPMI_ERR_INVALID_ARG; }
    const int64_t n = h->scan_map_n;
    if (h->d_stage_in.ensure(h, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    icpmi_status s = ops_transform_dev(h, correction, h->d_scan_map, n, h->d_stage_in); // Mapper.cpp:221
    if (s == ICPMI_OK) s = stage_chain_scalar(h, scan_scalar, n);
    if (s != ICPMI_OK) return s;
    return ops_map_update_chain(h, h->d_stage_in, n, nullptr, scan_scalar ? h->d_stage_s : nullptr, to_sensor, from_sensor, ops, n_ops, n_modules,
                                src_out, src_capacity, identity_prefix, new_m);
}

icpmi_status icpmi_set_map_scalar(icpmi_handle h, const float* scalar, int64_t m)
{
    CHECK_H(h);
    if (!scalar) { h->last_error = "set_map_scalar: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_map_scalar(h, scalar, nullptr, m);
}

icpmi_status icpmi_get_map_scalar(icpmi_handle h, float* scalar_out, int64_t capacity)
{
    CHECK_H(h);
    if (h->m <= 0 || h->m_raw == 0) return ICPMI_OK; // no map, or an empty resident map (a chain removed every point): nothing to
                                                     // hand out -- like icpmi_get_map, which reports 0 points
    if (!scalar_out || capacity < h->m_raw) { h->last_error = "get_map_scalar: no map, or capacity too small"; return ICPMI_ERR_INVALID_ARG; }
    return ops_map_scalar(h, nullptr, scalar_out, h->m_raw);
}

icpmi_status icpmi_get_map_densities(icpmi_handle h, float* densities_out, int64_t capacity)
{
    CHECK_H(h);
    return ops_get_map_densities(h, densities_out, capacity);
}

icpmi_status icpmi_max_density_keep(icpmi_handle h, const float* densities, int64_t n, float max_density, int32_t seed, uint8_t* keep)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!densities || !keep))) { h->last_error = "max_density_keep: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    if (!max_density_param_ok(max_density)) { h->last_error = "InvalidParameter: maxDensity must be finite and > 0"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffffll) { h->last_error = "max_density_keep: more than 2^31 - 1 points"; return ICPMI_ERR_UNSUPPORTED; }
    return ops_max_density_keep(h, densities, n, max_density, seed, keep);
}

icpmi_status icpmi_dynamic_points_update(icpmi_handle h, const icpmi_dynpts_params* prm, const float to_sensor[16], const float* in4,
                                         int64_t n, const float* map4, const float* map_normals3, int64_t m, float* prob_dynamic)
{
    CHECK_H(h);
    if (!prm || !to_sensor || n < 0 || m < 0 || (n > 0 && !in4) || (m > 0 && (!map4 || !map_normals3 || !prob_dynamic))) {
        h->last_error = "dynamic_points_update: bad arguments"; return ICPMI_ERR_INVALID_ARG;
    }
    if (!(prm->beam_half_angle > 0.f)) { h->last_error = "InvalidParameter: beamHalfAngle must be > 0"; return ICPMI_ERR_INVALID_ARG; }
    return ops_dynamic_points_update(h, prm, to_sensor, in4, n, map4, map_normals3, m, prob_dynamic);
}

icpmi_status icpmi_filter_points(icpmi_handle h, const float* in4, int64_t n, const icpmi_point_filter* filters, int32_t n_filters, uint8_t* keep)
{
    CHECK_H(h);
    if (n < 0 || n_filters < 0 || n_filters > ICPMI_MAX_POINT_FILTERS || (n_filters > 0 && !filters) || (n > 0 && (!in4 || !keep))) {
        h->last_error = "filter_points: bad arguments (at most 16 filters per call)"; return ICPMI_ERR_INVALID_ARG;
    }
    for (int32_t k = 0; k < n_filters; ++k) {
        const icpmi_point_filter& f = filters[k];
        if ((f.type != ICPMI_FILT_DISTANCE_LIMIT && f.type != ICPMI_FILT_BOUNDING_BOX) || (f.type == ICPMI_FILT_DISTANCE_LIMIT && (f.i < -1 || f.i > 2))) {
            h->last_error = "InvalidParameter: filter_points: unknown filter or dim outside [-1, 2]"; return ICPMI_ERR_INVALID_ARG;
        }
    }
    return ops_filter_points(h, in4, n, filters, n_filters, keep);
}

icpmi_status icpmi_sensor_model(icpmi_handle h, const float* in4, int64_t n, const float* normals3_in, const float* obs_dir3_in,
                                const icpmi_sensor_step* steps, int32_t n_steps, float* normals3_out, float* obs_dir3_out, float* noise_out,
                                uint8_t* keep_out)
{
    CHECK_H(h);
    if (n < 0 || n_steps < 0 || n_steps > ICPMI_MAX_SENSOR_STEPS || (n_steps > 0 && !steps) || (n > 0 && !in4)) {
        h->last_error = "sensor_model: bad arguments (at most 8 steps per call)"; return ICPMI_ERR_INVALID_ARG;
    }
    // what the program reads and produces, in chain order
    bool needs_n = false, needs_od_in = false, have_od = false, orient = false, shadow = false, noise = false, n_by_orient = false;
    for (int32_t k = 0; k < n_steps; ++k) {
        const icpmi_sensor_step& s = steps[k];
        switch (s.type) {
            case ICPMI_SM_OBSERVATION_DIRECTION: have_od = true; break;
            case ICPMI_SM_ORIENT_NORMALS: n_by_orient |= !needs_n; needs_n = orient = true; needs_od_in |= !have_od; break;
            case ICPMI_SM_SHADOW:
                if (!(s.f[0] >= 0.f && s.f[0] <= 1.f)) { h->last_error = "InvalidParameter: ShadowDataPointsFilter: eps must be in [0, 1]"; return ICPMI_ERR_INVALID_ARG; }
                needs_n = shadow = true;
                break;
            case ICPMI_SM_SIMPLE_SENSOR_NOISE:
                if (s.i < 0 || s.i > 4) { h->last_error = "InvalidParameter: SimpleSensorNoiseDataPointsFilter: sensorType must be 0 .. 4"; return ICPMI_ERR_INVALID_ARG; }
                if (!(s.f[0] > 0.f) || !std::isfinite(s.f[0])) { h->last_error = "InvalidParameter: SimpleSensorNoiseDataPointsFilter: gain must be finite and > 0"; return ICPMI_ERR_INVALID_ARG; }
                noise = true;
                break;
            default: h->last_error = "InvalidParameter: sensor_model: unknown step type"; return ICPMI_ERR_INVALID_ARG;
        }
    }
    if (n == 0) return ICPMI_OK;
    if (n > 0x7fffffffll) { h->last_error = "sensor_model: more than 2^31 - 1 points"; return ICPMI_ERR_UNSUPPORTED; }
    if (needs_n && !normals3_in) {
        h->last_error = n_by_orient ? "InvalidField: OrientNormalsDataPointsFilter: Error, cannot find normals in descriptors."
                               : "InvalidField: ShadowDataPointsFilter: Error, cannot find normals in descriptors";
        return ICPMI_ERR_MISSING_NORMALS;
    }
    if (needs_od_in && !obs_dir3_in) {
        h->last_error = "InvalidField: OrientNormalsDataPointsFilter: Error, cannot find observation directions in descriptors.";
        return ICPMI_ERR_INVALID_ARG;
    }
    if ((orient && !normals3_out) || (noise && !noise_out) || (shadow && !keep_out)) {
        h->last_error = "sensor_model: an output the program produces is NULL (normals3_out / noise_out / keep_out)"; return ICPMI_ERR_INVALID_ARG;
    }
    return ops_sensor_model(h, in4, n, needs_n ? normals3_in : nullptr, needs_od_in ? obs_dir3_in : nullptr, steps, n_steps, orient ? normals3_out : nullptr,
                            have_od ? obs_dir3_out : nullptr, noise ? noise_out : nullptr, shadow ? keep_out : nullptr);
}

icpmi_status icpmi_deskew_table(const icpmi_sweep_motion* m, float* q4, float* p3, float* omega, float* inv_sin)
{
    return deskew_table_host(m, q4, p3, omega, inv_sin, g_create_error); // (no handle: icpmi_last_error(NULL) has the message)
}

icpmi_status icpmi_deskew(icpmi_handle h, const float* in4, int64_t n, const float* t_rel, const icpmi_sweep_motion* m, float* out4,
                          const float* in_normals3, float* out_normals3)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!in4 || !t_rel || !out4 || (in_normals3 != nullptr) != (out_normals3 != nullptr)))) {
        h->last_error = "deskew: bad arguments (in4, t_rel and out4 are needed; the normals come in and out together)"; return ICPMI_ERR_INVALID_ARG;
    }
    return ops_deskew(h, in4, n, t_rel, m, out4, in_normals3, out_normals3, false);
}

icpmi_status icpmi_deskew_dev(icpmi_handle h, const float* d_in4, int64_t n, const float* d_t_rel, const icpmi_sweep_motion* m, float* d_out4,
                              const float* d_in_normals3, float* d_out_normals3)
{
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!d_in4 || !d_t_rel || !d_out4 || (d_in_normals3 != nullptr) != (d_out_normals3 != nullptr)))) {
        h->last_error = "deskew_dev: bad arguments (d_in4, d_t_rel and d_out4 are needed; the normals come in and out together)"; return ICPMI_ERR_INVALID_ARG;
    }
    return ops_deskew(h, d_in4, n, d_t_rel, m, d_out4, d_in_normals3, d_out_normals3, true);
}

// ---- sweep registration (include/icpmi.h: icpmi_register_sweep; csrc/sweep.hip) ----
void icpmi_sweep_options_default(icpmi_sweep_options* opts)
{
    if (!opts) return;
    memset(opts, 0, sizeof *opts);
    opts->begin_s = 0.0; opts->end_s = 0.1; opts->time_unit_s = 1e-9;
    opts->max_iterations = 12;
    opts->min_step_rot = -1.f; opts->min_step_trans = -1.f;
}

icpmi_status icpmi_sweep_solve(const double sums80[80], double lambda_rot, double lambda_trans, const double d6[6], double x12[12])
{
    return sweep_solve_host(sums80, lambda_rot, lambda_trans, d6, x12, g_create_error); // (no handle: icpmi_last_error(NULL) has the message)
}

// icpmi_register_sweep* (sums80 == nullptr) and icpmi_sweep_sums: the refusals of the path, the chain's set-up, the call.  Device pointers.
static icpmi_status sweep_impl(icpmi_handle h, const char* who, const float* d_scan4, int64_t n, const float* d_t_rel, const float* T_begin,
                               const float* T_end, const icpmi_sweep_options* opts, icpmi_sweep_result* result, float* d_out4, double* sums80)
{
    const int64_t have_scalar_n = h->read_scalar_n, have_r2_n = h->read_r2_n;
    h->read_scalar_n = 0; h->read_noise_n = 0; h->read_r2_n = 0; h->read_int_n = 0;
    if (result) { memset(result, 0, sizeof *result); result->trimmed_limit = -1.f; }
    if (sums80) memset(sums80, 0, 80 * sizeof(double));
    if (n < 0 || (n > 0 && (!d_scan4 || !d_t_rel)) || !T_begin || !T_end || (!sums80 && !result) || (sums80 && n < 1) ||
        (d_out4 && d_out4 == d_scan4)) {
        h->last_error = std::string(who) + ": bad arguments"; return ICPMI_ERR_INVALID_ARG;
    }
    { const icpmi_status os = sweep_check_options(opts, h->last_error); if (os != ICPMI_OK) return os; }
    { const icpmi_status is = reject_intensity(h, who); if (is != ICPMI_OK) return is; }
    { const icpmi_status vs = voxel_check(h, who, false); if (vs != ICPMI_OK) return vs; }
    const icpmi_config& cfg = h->cfg;
    if (cfg.force_4dof || cfg.force_2d || cfg.is_2d || cfg.covariance || cfg.degeneracy_threshold != 0.f) {
        h->last_error = std::string(who) + ": not served with force_4dof, force_2d, is_2d, covariance or a degeneracy_threshold"; return ICPMI_ERR_INVALID_ARG;
    }
    if (cfg.minimizer != ICPMI_MIN_POINT_TO_PLANE) {
        h->last_error = std::string(who) + ": served for PointToPlaneErrorMinimizer only"; return ICPMI_ERR_INVALID_ARG;
    }
    { const icpmi_status rs = check_rigid(h, T_begin); if (rs != ICPMI_OK) return rs; }
    { const icpmi_status rs = check_rigid(h, T_end); if (rs != ICPMI_OK) return rs; }
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T_begin[i]) || !std::isfinite(T_end[i])) { h->last_error = std::string(who) + ": a non-finite prior"; return ICPMI_ERR_INVALID_ARG; }
    if (n == 0) { sweep_result_priors(T_begin, T_end, result); return ICPMI_OK; }
    if (h->m <= 0) { h->last_error = std::string(who) + ": no map"; return ICPMI_ERR_INVALID_ARG; }
    if (n > 0x7fffffff / ICPMI_MAX_K) { h->last_error = std::string(who) + ": too many points"; return ICPMI_ERR_UNSUPPORTED; }
    int32_t kind = ICPMI_RES_POINT_TO_PLANE; // (without map normals: ICPMI_ERR_MISSING_NORMALS)
    LoopCfg lc;
    const float* d_r2row = nullptr;
    bool needs_rn = false;
    { const icpmi_status cs = residual_chain_setup(h, who, n, nullptr, have_scalar_n, have_r2_n, &kind, &lc, &d_r2row, &needs_rn); if (cs != ICPMI_OK) return cs; }
    if (sums80) return sweep_sums_dev(h, (const float4*)d_scan4, n, d_t_rel, lc, d_r2row, T_begin, T_end, opts, sums80, result);
    return sweep_register_dev(h, (const float4*)d_scan4, n, d_t_rel, lc, d_r2row, T_begin, T_end, opts, result, (float4*)d_out4);
}

// the host-pointer calls: scan, point times and (want_out) the deskewed scan in scratch slot 22, [n float4][n float4][n float]
static icpmi_status sweep_stage(icpmi_ctx* h, const float* scan4, int64_t n, const float* t_rel, const float** d_scan, const float** d_t, float** d_out)
{
    float4* blk = scratch_get<float4>(h, 22, (size_t)2 * n + ((size_t)n + 3) / 4);
    if (!blk) return ICPMI_ERR_HIP;
    HIP_TRY(h, hipMemcpyAsync(blk, scan4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(blk + 2 * n, t_rel, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    *d_scan = (const float*)blk; *d_out = (float*)(blk + n); *d_t = (const float*)(blk + 2 * n);
    return ICPMI_OK;
}

icpmi_status icpmi_register_sweep_dev(icpmi_handle h, const float* d_scan4, int64_t n, const float* d_t_rel, const float prior_begin16[16],
                                      const float prior_end16[16], const icpmi_sweep_options* opts, icpmi_sweep_result* result, float* d_out4)
{
    CHECK_H(h);
    return sweep_impl(h, "register_sweep_dev", d_scan4, n, d_t_rel, prior_begin16, prior_end16, opts, result, d_out4, nullptr);
}

icpmi_status icpmi_register_sweep(icpmi_handle h, const float* scan4, int64_t n, const float* t_rel, const float prior_begin16[16],
                                  const float prior_end16[16], const icpmi_sweep_options* opts, icpmi_sweep_result* result, float* out4)
{
    CHECK_H(h);
    const float* d_scan = scan4; const float* d_t = t_rel; float* d_out = nullptr; // (n == 0, no map or bad arguments: never dereferenced)
    if (n > 0 && scan4 && t_rel && h->m > 0) { const icpmi_status ss = sweep_stage(h, scan4, n, t_rel, &d_scan, &d_t, &d_out); if (ss != ICPMI_OK) return ss; }
    const icpmi_status s = sweep_impl(h, "register_sweep", d_scan, n, d_t, prior_begin16, prior_end16, opts, result, out4 ? d_out : nullptr, nullptr);
    // (staged or not, the stream is drained: the caller's arrays are free on every return)
    if (s != ICPMI_OK) { (void)hipStreamSynchronize(h->stream); return s; }
    if (out4 && n > 0 && d_out) HIP_TRY(h, hipMemcpyAsync(out4, d_out, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return ICPMI_OK;
}

icpmi_status icpmi_sweep_sums(icpmi_handle h, const float* scan4, int64_t n, const float* t_rel, const float T_begin16[16], const float T_end16[16],
                              const icpmi_sweep_options* opts, double sums80[80], icpmi_sweep_result* stats)
{
    CHECK_H(h);
    if (!sums80) { h->last_error = "sweep_sums: sums80 is NULL"; return ICPMI_ERR_INVALID_ARG; }
    const float* d_scan = scan4; const float* d_t = t_rel; float* d_out = nullptr;
    if (n > 0 && scan4 && t_rel && h->m > 0) { const icpmi_status ss = sweep_stage(h, scan4, n, t_rel, &d_scan, &d_t, &d_out); if (ss != ICPMI_OK) return ss; }
    const icpmi_status s = sweep_impl(h, "sweep_sums", d_scan, n, d_t, T_begin16, T_end16, opts, stats, nullptr, sums80);
    (void)hipStreamSynchronize(h->stream);
    return s;
}

icpmi_status icpmi_bin_cells(icpmi_handle h, const float* pts4, int64_t n, float cell_size, int32_t* ijk3)
{
    CHECK_H(h);
    if (n < 0 || !(cell_size > 0.f) || (n > 0 && (!pts4 || !ijk3))) { h->last_error = "bin_cells: bad arguments"; return ICPMI_ERR_INVALID_ARG; }
    return ops_bin_cells(h, pts4, n, cell_size, ijk3);
}

} // extern "C"
