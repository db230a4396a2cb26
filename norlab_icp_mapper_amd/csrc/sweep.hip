// sweep.hip -- sweep registration: the sensor's motion within one scan estimated by ICP (include/icpmi.h: icpmi_register_sweep has the
// formulation).  Two poses, sweep begin and sweep end, are estimated by the chain's own matcher and outlier filters; every
// pair's Jacobian is split between them by the pair's point time.
//
// One iteration is built from launches the tree already has -- deskew_kernel (deskew.hip) out of place into a work buffer, then the
// one-pass front of loop_residual (loop.hip: centring + tile sort, fresh state, the matcher's launch, the selections) -- and two kernels
// of its own: sweep_pairs_kernel walks the pairs through walk_pairs and sums the time moments of the point-to-plane normal equations in
// double, one row of partials per workgroup; sweep_finish_kernel adds the rows in a fixed order.  No atomics.  The 12 x 12 system is
// solved on the host in double (sweep_solve_host: a pure function), where the two poses live as translation + quaternion.
//
// Registers (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md 4.18 has the figures; the 78 double
// accumulators of sweep_pairs_kernel stay in registers (no scratch).
#include "common.h"

#include <cmath>
#include <cstring>

namespace {

#define ICPMI_SW_NB 256   // pass-1 workgroups, one per CU (fixed, as ICPMI_RES_NB: the summation order depends on the slot count alone)
#define ICPMI_SW_NV 78    // the values of icpmi_sweep_sums' sums[80] that are summed; [78], [79] are written as zero
#define ICPMI_SW_CH 8     // pass 2: eight threads per value, each over every eighth row of partials
#define ICPMI_SW_M0 0
#define ICPMI_SW_M1 21
#define ICPMI_SW_M2 42
#define ICPMI_SW_G0 63
#define ICPMI_SW_G1 69
#define ICPMI_SW_W 75
#define ICPMI_SW_PAIRS 76
#define ICPMI_SW_WR2 77

// what one pass hands to the host in one copy
struct SweepBlock { double sums[80]; float limit; int error; };

// alpha_i = clamp((t_rel[i] * unit - begin) / (end - begin), 0, 1) in double, rounded once (deskew_kernel's u for the two-stamp table
// {begin, end} with extrapolate set: the same expressions); a NaN raises the flag with an ordinary store of the constant 1
__global__ __launch_bounds__(256) void sweep_alpha_kernel(const float* __restrict__ t_rel, int64_t n, double unit, double begin_s, double end_s,
                                                          float* __restrict__ alpha, unsigned* flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double tau = (double)t_rel[i] * unit;
    if (tau != tau) { *flag = 1u; alpha[i] = 0.f; return; }
    tau = tau < begin_s ? begin_s : (tau > end_s ? end_s : tau);
    alpha[i] = (float)((tau - begin_s) / (end_s - begin_s));
}

// fused_slot >= 0: the chain's one quantile filter went through the fused selection; every workgroup resolves its last level, as
// res_pairs_kernel does (the same lookup, the same limit).  alpha: by the reading's ORIGINAL index (the pairs arrive tile-sorted).
__global__ __launch_bounds__(256) void sweep_pairs_kernel(PairView pv, int n, LoopCfg lc, IcpState* __restrict__ st, const unsigned* __restrict__ hists,
                                                          int fused_slot, int is_median, float factor, const float* __restrict__ alpha,
                                                          double* __restrict__ partial)
{
    __shared__ unsigned shsel[16];
    float fused_limit = 0.f;
    if (fused_slot >= 0) {
        const unsigned cv = hists[ICPMI_S2_C1 + threadIdx.x];
        unsigned bin, rem, total;
        block_find_rank_2tier<1>(cv, hists + ICPMI_S2_F1, false, 0.f, st->sel_rank_l[0], shsel, bin, rem, total);
        const float q = __uint_as_float((st->sel_prefix_l[0] << 16) | bin);
        fused_limit = is_median ? factor * q : q;
        if (blockIdx.x == 0 && threadIdx.x == 0) st->limits[fused_slot] = fused_limit;
    }
    double acc[ICPMI_SW_NV];
#pragma unroll
    for (int i = 0; i < ICPMI_SW_NV; ++i) acc[i] = 0.0;
    if (st->error == 0) // (otherwise a selection that found nothing to filter: the partials are written, all zero)
        walk_pairs(pv, n, lc, st, st->T_iter, [&](const PairSlot& s) {
            if (s.w == 0.f) return;
            // per-pair quantities in float exactly as the point-to-plane pair sums form them (loop.hip: accumulate_kernel)
            const float F[6] = {s.p.y * s.nm.z - s.p.z * s.nm.y, s.p.z * s.nm.x - s.p.x * s.nm.z, s.p.x * s.nm.y - s.p.y * s.nm.x, s.nm.x, s.nm.y, s.nm.z};
            const double a = (double)alpha[s.oi], a2 = a * a;
            int idx = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double wf = (double)s.w * F[i];
#pragma unroll
                for (int j = i; j < 6; ++j) {
                    const double m = wf * F[j];
                    acc[ICPMI_SW_M0 + idx] += m; acc[ICPMI_SW_M1 + idx] += a * m; acc[ICPMI_SW_M2 + idx] += a2 * m;
                    ++idx;
                }
                const double gr = wf * s.dot;
                acc[ICPMI_SW_G0 + i] += gr; acc[ICPMI_SW_G1 + i] += a * gr;
            }
            acc[ICPMI_SW_W] += (double)s.w; acc[ICPMI_SW_PAIRS] += 1.0;
            acc[ICPMI_SW_WR2] += ((double)s.w * s.dot) * s.dot;
        }, fused_slot, fused_limit);
    block_partial_row<ICPMI_SW_NV>(acc, partial + (size_t)blockIdx.x * ICPMI_SW_NV);
}

// one workgroup of ICPMI_SW_NV * ICPMI_SW_CH <= 640 threads: value v = the sum over c = 0 .. 7, in order, of the sums over i = 0 .. 31, in
// order, of row c + 8 i (block_ordered_total)
__global__ __launch_bounds__(640) void sweep_finish_kernel(const double* __restrict__ partial, const IcpState* __restrict__ st, int limit_slot,
                                                           SweepBlock* __restrict__ out)
{
    __shared__ double tot[ICPMI_SW_NV];
    block_ordered_total<ICPMI_SW_NV, ICPMI_SW_CH, ICPMI_SW_NB>(partial, ICPMI_SW_NB, tot);
    if (threadIdx.x < 80) out->sums[threadIdx.x] = threadIdx.x < ICPMI_SW_NV ? tot[threadIdx.x] : 0.0;
    if (threadIdx.x == 0) {
        out->limit = limit_slot >= 0 ? st->limits[limit_slot] : -1.f;
        out->error = st->error;
    }
}
static_assert(ICPMI_SW_NB % ICPMI_SW_CH == 0 && ICPMI_SW_NV * ICPMI_SW_CH <= 640, "pass 2 of the sweep sums: one workgroup, whole chunks");

// ---- the two poses on the host: translation + unit quaternion (x y z w), double ----
struct Pose { double t[3]; double q[4]; };

void quat_normalise(double q[4])
{
    const double s = 1.0 / std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] *= s;
}
void quat_rot(const double q[4], double R[3][3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - w * z); R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z); R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y); R[2][1] = 2.0 * (y * z + w * x); R[2][2] = 1.0 - 2.0 * (x * x + y * y);
}
// a column-major 4 x 4 whose rotation part passed check_rigid (Shepperd's choice of the largest component)
Pose pose_from_T(const float T[16])
{
    Pose P;
    double R[3][3];
    for (int r = 0; r < 3; ++r) { P.t[r] = T[12 + r]; for (int c = 0; c < 3; ++c) R[r][c] = T[4 * c + r]; }
    const double tr = R[0][0] + R[1][1] + R[2][2];
    double* q = P.q;
    if (tr > 0.0) {
        const double s = 2.0 * std::sqrt(1.0 + tr);
        q[3] = 0.25 * s; q[0] = (R[2][1] - R[1][2]) / s; q[1] = (R[0][2] - R[2][0]) / s; q[2] = (R[1][0] - R[0][1]) / s;
    } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
        const double s = 2.0 * std::sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]);
        q[3] = (R[2][1] - R[1][2]) / s; q[0] = 0.25 * s; q[1] = (R[0][1] + R[1][0]) / s; q[2] = (R[0][2] + R[2][0]) / s;
    } else if (R[1][1] > R[2][2]) {
        const double s = 2.0 * std::sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]);
        q[3] = (R[0][2] - R[2][0]) / s; q[0] = (R[0][1] + R[1][0]) / s; q[1] = 0.25 * s; q[2] = (R[1][2] + R[2][1]) / s;
    } else {
        const double s = 2.0 * std::sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]);
        q[3] = (R[1][0] - R[0][1]) / s; q[0] = (R[0][2] + R[2][0]) / s; q[1] = (R[1][2] + R[2][1]) / s; q[2] = 0.25 * s;
    }
    quat_normalise(q);
    return P;
}
void pose_to_T(const Pose& P, float T[16])
{
    double R[3][3];
    quat_rot(P.q, R);
    for (int c = 0; c < 3; ++c) { for (int r = 0; r < 3; ++r) T[4 * c + r] = (float)R[r][c]; T[4 * c + 3] = 0.f; }
    for (int r = 0; r < 3; ++r) T[12 + r] = (float)P.t[r];
    T[15] = 1.f;
}
// the pose in the centred frame, [R | t + R mu - mu], formed in double
void pose_centred(const Pose& P, const float mean[3], float Tc[16])
{
    double R[3][3];
    quat_rot(P.q, R);
    for (int c = 0; c < 3; ++c) { for (int r = 0; r < 3; ++r) Tc[4 * c + r] = (float)R[r][c]; Tc[4 * c + 3] = 0.f; }
    for (int r = 0; r < 3; ++r)
        Tc[12 + r] = (float)((P.t[r] + ((R[r][0] * (double)mean[0] + R[r][1] * (double)mean[1]) + R[r][2] * (double)mean[2])) - (double)mean[r]);
    Tc[15] = 1.f;
}
// ... of a pose given as a float 4 x 4: the expression of icpmi_residual_error (api.hip: centred_pose), so that icpmi_sweep_sums matches
// under the bits icpmi_residual_error and icpmi_minimize_step match under
void matrix_centred(const float T[16], const float mean[3], float Tc[16])
{
    memcpy(Tc, T, 16 * sizeof(float));
    for (int r = 0; r < 3; ++r)
        Tc[12 + r] = (float)(((double)T[12 + r] + (((double)T[r] * (double)mean[0] + (double)T[4 + r] * (double)mean[1]) + (double)T[8 + r] * (double)mean[2])) -
                             (double)mean[r]);
    Tc[3] = Tc[7] = Tc[11] = 0.f; Tc[15] = 1.f;
}
// P <- S(xi) P with the centred-frame step xi = (omega, t) moved to the map frame: S = [R_s | t + mu - R_s mu], R_s = exp([omega]x)
void pose_apply_step(Pose& P, const double xi[6], const float mean[3])
{
    const double th = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    double qs[4] = {0.5 * xi[0], 0.5 * xi[1], 0.5 * xi[2], 1.0}; // (th -> 0: sin(th / 2) / th -> 1 / 2)
    if (th > 1e-12) { const double k = std::sin(0.5 * th) / th; qs[0] = k * xi[0]; qs[1] = k * xi[1]; qs[2] = k * xi[2]; qs[3] = std::cos(0.5 * th); }
    quat_normalise(qs);
    double R[3][3];
    quat_rot(qs, R);
    const double d[3] = {P.t[0] - (double)mean[0], P.t[1] - (double)mean[1], P.t[2] - (double)mean[2]};
    for (int r = 0; r < 3; ++r) P.t[r] = (((R[r][0] * d[0] + R[r][1] * d[1]) + R[r][2] * d[2]) + xi[3 + r]) + (double)mean[r];
    const double* a = qs; const double b[4] = {P.q[0], P.q[1], P.q[2], P.q[3]}; // Hamilton product: the rotation of b, then of a
    P.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    P.q[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    P.q[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    P.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    quat_normalise(P.q);
}

// the device blocks of a call: everything is allocated before the first launch
struct SweepBufs {
    float4* d_work = nullptr;        // the deskewed scan (slot 20)
    float* d_alpha = nullptr;        // slot 21
    double* d_part = nullptr;        // slot 23: [partials][SweepBlock][T0: 16 floats][flag word, padded][the deskew table: ICPMI_UP_SLOT bytes]
    SweepBlock* d_block = nullptr;
    float* d_T0 = nullptr;
    unsigned* d_flag = nullptr;
    unsigned char* d_tab = nullptr;
};
constexpr size_t SW_BLOCK_DOUBLES = (sizeof(SweepBlock) + sizeof(double) - 1) / sizeof(double);

icpmi_status sweep_bufs(icpmi_ctx* c, int64_t n, const LoopCfg& lc, SweepBufs& B)
{
    if (ensure_loop_buffers(c, n, lc) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (c->d_reading.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    B.d_work = scratch_get<float4>(c, 20, (size_t)n + 1);
    B.d_alpha = scratch_get<float>(c, 21, (size_t)n);
    constexpr size_t PART = (size_t)ICPMI_SW_NB * ICPMI_SW_NV, OFF_T0 = PART + SW_BLOCK_DOUBLES, OFF_FLAG = OFF_T0 + 8,
                     OFF_TAB = (OFF_FLAG + 1 + 1) & ~(size_t)1; // (the table holds float4 rows: 16-byte aligned)
    B.d_part = scratch_get<double>(c, 23, OFF_TAB + ICPMI_UP_SLOT / sizeof(double));
    if (!B.d_work || !B.d_alpha || !B.d_part) return ICPMI_ERR_HIP;
    B.d_block = reinterpret_cast<SweepBlock*>(B.d_part + PART);
    B.d_T0 = reinterpret_cast<float*>(B.d_part + OFF_T0);
    B.d_flag = reinterpret_cast<unsigned*>(B.d_part + OFF_FLAG);
    B.d_tab = reinterpret_cast<unsigned char*>(B.d_part + OFF_TAB);
    return ICPMI_OK;
}

// the point times -> alpha; waits for the NaN flag
icpmi_status sweep_alpha(icpmi_ctx* c, const SweepBufs& B, const float* d_t_rel, int64_t n, const icpmi_sweep_options* o)
{
    HIP_TRY(c, hipMemsetAsync(B.d_flag, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(sweep_alpha_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_t_rel, n, o->time_unit_s, o->begin_s, o->end_s,
                       B.d_alpha, B.d_flag);
    HIP_TRY(c, hipGetLastError());
    unsigned flag = 0;
    if (read_back(c, &flag, B.d_flag, sizeof flag) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (flag) { c->last_error = "register_sweep: a point time is NaN"; return ICPMI_ERR_INVALID_ARG; }
    return ICPMI_OK;
}

icpmi_status sweep_deskew(icpmi_ctx* c, const SweepBufs& B, const float4* d_scan, int64_t n, const float* d_t_rel, const Pose& Pb, const Pose& Pe,
                          const icpmi_sweep_options* o, float4* d_out)
{
    const double stamps[2] = {o->begin_s, o->end_s};
    const double pose7[14] = {Pb.t[0], Pb.t[1], Pb.t[2], Pb.q[0], Pb.q[1], Pb.q[2], Pb.q[3], Pe.t[0], Pe.t[1], Pe.t[2], Pe.q[0], Pe.q[1], Pe.q[2], Pe.q[3]};
    icpmi_sweep_motion m;
    m.n_poses = 2; m.extrapolate = 1; m.stamp_s = stamps; m.pose7 = pose7; m.ref_s = o->end_s; m.time_unit_s = o->time_unit_s; m.round_s = 0.0;
    return deskew_enqueue_dev(c, d_scan, n, d_t_rel, &m, B.d_tab, d_out);
}

// steps 1 to 4 of one iteration.  Tc: the end pose in the centred frame
icpmi_status sweep_pass(icpmi_ctx* c, const SweepBufs& B, const float4* d_scan, int64_t n, const float* d_t_rel, const LoopCfg& lc, const float* d_r2row,
                        const Pose& Pb, const Pose& Pe, const float Tc[16], const icpmi_sweep_options* o, SweepBlock* hb)
{
    { const icpmi_status s = sweep_deskew(c, B, d_scan, n, d_t_rel, Pb, Pe, o, B.d_work); if (s != ICPMI_OK) return s; }
    { const icpmi_status s = loop_prepare_reading(c, B.d_work, n, nullptr); if (s != ICPMI_OK) return s; }
    { const icpmi_status s = upload_small(c, B.d_T0, Tc, 16 * sizeof(float)); if (s != ICPMI_OK) return s; }
    { const icpmi_status s = enqueue_fresh_states(c, 1, B.d_T0); if (s != ICPMI_OK) return s; }
    const LoopCfg l1 = one_pass_cfg(lc);
    const NnRequest req = loop_request(c, l1, batch_of_one(n), d_r2row); // (iter 0: what a registration's first iteration asks of the matcher)
    NnOutcome nn;
    { const icpmi_status s = enqueue_match_select(c, n, l1, req, &nn); if (s != ICPMI_OK) return s; }
    const int slot = fused_filter_slot(l1);
    hipLaunchKernelGGL(sweep_pairs_kernel, dim3(ICPMI_SW_NB), dim3(256), 0, c->stream, pair_view(c, l1, nn.out_sorted), (int)n, l1, c->d_state,
                       (const unsigned*)c->d_selhist, slot >= 0 ? slot : -1, (slot >= 0 && l1.out_type[slot] == ICPMI_OUT_MEDIANDIST) ? 1 : 0,
                       slot >= 0 ? l1.out_param[slot] : 0.f, (const float*)B.d_alpha, B.d_part);
    hipLaunchKernelGGL(sweep_finish_kernel, dim3(1), dim3(640), 0, c->stream, (const double*)B.d_part, (const IcpState*)c->d_state, quantile_slot(l1),
                       B.d_block);
    HIP_TRY(c, hipGetLastError());
    if (read_back(c, hb, B.d_block, sizeof *hb) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (hb->error) {
        c->last_error = hb->error == ICPMI_ERR_NO_OUTLIER_TO_FILTER ? "ConvergenceError: no outlier to filter" : "register_sweep: device-side convergence error";
        return (icpmi_status)hb->error;
    }
    return ICPMI_OK;
}

void sweep_result(const Pose& Pb, const Pose& Pe, const SweepBlock* hb, int k, int64_t n, int iterations, int stop, icpmi_sweep_result* res)
{
    if (!res) return;
    memset(res, 0, sizeof *res);
    pose_to_T(Pb, res->T_begin); pose_to_T(Pe, res->T_end);
    for (int i = 0; i < 3; ++i) { res->pose7[i] = Pb.t[i]; res->pose7[7 + i] = Pe.t[i]; }
    for (int i = 0; i < 4; ++i) { res->pose7[3 + i] = Pb.q[i]; res->pose7[10 + i] = Pe.q[i]; }
    res->iterations = iterations; res->stop_reason = stop;
    res->trimmed_limit = -1.f;
    if (!hb) return;
    res->pairs = (int64_t)hb->sums[ICPMI_SW_PAIRS];
    res->weight_sum = hb->sums[ICPMI_SW_W];
    res->sum_sq = hb->sums[ICPMI_SW_WR2];
    res->weighted_point_used_ratio = (float)(hb->sums[ICPMI_SW_W] / ((double)k * (double)n));
    res->trimmed_limit = hb->limit;
}

// a registration's covariance and localizability report do not survive the matcher's launches of this path
void sweep_drop_reports(icpmi_ctx* c) { c->cov_ready = false; c->cov_kept = false; c->degen_ready = false; }

} // namespace

// the result of a call that ran no iteration (no points): the priors as they came, and their double form
void sweep_result_priors(const float T_begin[16], const float T_end[16], icpmi_sweep_result* res)
{
    sweep_result(pose_from_T(T_begin), pose_from_T(T_end), nullptr, 1, 0, 0, 0, res);
    memcpy(res->T_begin, T_begin, sizeof res->T_begin); memcpy(res->T_end, T_end, sizeof res->T_end);
}

icpmi_status sweep_check_options(const icpmi_sweep_options* o, std::string& err)
{
    if (!o) { err = "register_sweep: opts is NULL"; return ICPMI_ERR_INVALID_ARG; }
    if (!std::isfinite(o->begin_s) || !std::isfinite(o->end_s) || !std::isfinite(o->time_unit_s) || !std::isfinite(o->lambda_rot) ||
        !std::isfinite(o->lambda_trans) || !std::isfinite(o->min_step_rot) || !std::isfinite(o->min_step_trans)) {
        err = "register_sweep: a non-finite option"; return ICPMI_ERR_INVALID_ARG;
    }
    if (!(o->begin_s < o->end_s)) { err = "register_sweep: begin_s must be < end_s"; return ICPMI_ERR_INVALID_ARG; }
    if (!(o->time_unit_s > 0.0)) { err = "register_sweep: time_unit_s must be > 0"; return ICPMI_ERR_INVALID_ARG; }
    if (o->lambda_rot < 0.0 || o->lambda_trans < 0.0) { err = "register_sweep: the prior weights must be >= 0"; return ICPMI_ERR_INVALID_ARG; }
    if (o->max_iterations < 1) { err = "register_sweep: max_iterations must be >= 1"; return ICPMI_ERR_INVALID_ARG; }
    return ICPMI_OK;
}

// step 5's system (include/icpmi.h): factored in the variables (xi_b, delta = xi_e - xi_b), where it reads
// [[M0, M1], [M1, M2 + L]] (xi_b ; delta) = [-g0 ; -g1 - L d]
icpmi_status sweep_solve_host(const double sums[80], double lambda_rot, double lambda_trans, const double* d6, double x12[12], std::string& err)
{
    if (!sums || !x12) { err = "sweep_solve: a NULL argument"; return ICPMI_ERR_INVALID_ARG; }
    for (int i = 0; i < 12; ++i) x12[i] = 0.0;
    if (!std::isfinite(lambda_rot) || !std::isfinite(lambda_trans) || lambda_rot < 0.0 || lambda_trans < 0.0) {
        err = "sweep_solve: the prior weights must be finite and >= 0"; return ICPMI_ERR_INVALID_ARG;
    }
    if (!(sums[ICPMI_SW_PAIRS] > 0.0)) { err = "ConvergenceError: ErrorMinimizer: no point to minimize"; return ICPMI_ERR_NO_POINT_TO_MINIMIZE; }
    double A[12][12], y[12];
    int idx = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++idx) {
            A[i][j] = A[j][i] = sums[ICPMI_SW_M0 + idx];
            A[i][6 + j] = A[j][6 + i] = A[6 + i][j] = A[6 + j][i] = sums[ICPMI_SW_M1 + idx];
            A[6 + i][6 + j] = A[6 + j][6 + i] = sums[ICPMI_SW_M2 + idx];
        }
    for (int i = 0; i < 6; ++i) {
        const double L = sums[ICPMI_SW_W] * (i < 3 ? lambda_rot : lambda_trans);
        A[6 + i][6 + i] += L;
        y[i] = -sums[ICPMI_SW_G0 + i];
        y[6 + i] = -sums[ICPMI_SW_G1 + i] - L * (d6 ? d6[i] : 0.0);
    }
    double dmax = 0.0;
    for (int i = 0; i < 12; ++i) dmax = std::fmax(dmax, A[i][i]);
    // Cholesky A = G G^T, G in the lower triangle
    for (int j = 0; j < 12; ++j) {
        double piv = A[j][j];
        for (int k = 0; k < j; ++k) piv -= A[j][k] * A[j][k];
        if (!(piv > 1e-12 * dmax)) { // (a NaN among the sums ends here too)
            err = "register_sweep: the motion within the sweep is not observable from these pairs (a pivot of the 12 x 12 system vanishes): "
                  "a prior weight (lambda_rot, lambda_trans) is needed";
            return ICPMI_ERR_NAN;
        }
        const double g = std::sqrt(piv);
        A[j][j] = g;
        for (int i = j + 1; i < 12; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
            A[i][j] = v / g;
        }
    }
    for (int i = 0; i < 12; ++i) { double v = y[i]; for (int k = 0; k < i; ++k) v -= A[i][k] * y[k]; y[i] = v / A[i][i]; }
    for (int i = 11; i >= 0; --i) { double v = y[i]; for (int k = i + 1; k < 12; ++k) v -= A[k][i] * y[k]; y[i] = v / A[i][i]; }
    for (int i = 0; i < 6; ++i) { x12[i] = y[i]; x12[6 + i] = y[i] + y[6 + i]; }
    return ICPMI_OK;
}

icpmi_status sweep_sums_dev(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_t_rel, const LoopCfg& lc, const float* d_r2row,
                            const float T_begin[16], const float T_end[16], const icpmi_sweep_options* opts, double sums[80], icpmi_sweep_result* res)
{
    sweep_drop_reports(c);
    SweepBufs B;
    { const icpmi_status s = sweep_bufs(c, n, lc, B); if (s != ICPMI_OK) return s; }
    { const icpmi_status s = sweep_alpha(c, B, d_t_rel, n, opts); if (s != ICPMI_OK) return s; }
    const Pose Pb = pose_from_T(T_begin), Pe = pose_from_T(T_end);
    float Tc[16];
    matrix_centred(T_end, c->mean, Tc);
    SweepBlock hb;
    { const icpmi_status s = sweep_pass(c, B, d_scan, n, d_t_rel, lc, d_r2row, Pb, Pe, Tc, opts, &hb); if (s != ICPMI_OK) return s; }
    if (sums) memcpy(sums, hb.sums, sizeof hb.sums);
    sweep_result(Pb, Pe, &hb, lc.k, n, 0, 0, res);
    if (res) { memcpy(res->T_begin, T_begin, sizeof res->T_begin); memcpy(res->T_end, T_end, sizeof res->T_end); }
    return ICPMI_OK;
}

icpmi_status sweep_register_dev(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_t_rel, const LoopCfg& lc, const float* d_r2row,
                                const float T_begin[16], const float T_end[16], const icpmi_sweep_options* opts, icpmi_sweep_result* res, float4* d_out4)
{
    sweep_drop_reports(c);
    SweepBufs B;
    { const icpmi_status s = sweep_bufs(c, n, lc, B); if (s != ICPMI_OK) return s; }
    { const icpmi_status s = sweep_alpha(c, B, d_t_rel, n, opts); if (s != ICPMI_OK) return s; }
    Pose Pb = pose_from_T(T_begin), Pe = pose_from_T(T_end);
    const double min_rot = opts->min_step_rot < 0.f ? (double)c->cfg.min_diff_rot : (double)opts->min_step_rot;
    const double min_trans = opts->min_step_trans < 0.f ? (double)c->cfg.min_diff_trans : (double)opts->min_step_trans;
    double d[6] = {0, 0, 0, 0, 0, 0}; // the relative motion's increment so far: the sum of xi_e - xi_b
    SweepBlock hb;
    int it = 0, stop = ICPMI_STOP_COUNTER;
    while (it < opts->max_iterations) {
        float Tc[16];
        pose_centred(Pe, c->mean, Tc);
        { const icpmi_status s = sweep_pass(c, B, d_scan, n, d_t_rel, lc, d_r2row, Pb, Pe, Tc, opts, &hb); if (s != ICPMI_OK) return s; }
        double x[12];
        { const icpmi_status s = sweep_solve_host(hb.sums, opts->lambda_rot, opts->lambda_trans, d, x, c->last_error); if (s != ICPMI_OK) return s; }
        pose_apply_step(Pb, x, c->mean);
        pose_apply_step(Pe, x + 6, c->mean);
        for (int i = 0; i < 6; ++i) d[i] += x[6 + i] - x[i];
        ++it;
        const auto norm3 = [](const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
        if (norm3(x) < min_rot && norm3(x + 3) < min_trans && norm3(x + 6) < min_rot && norm3(x + 9) < min_trans) { stop = ICPMI_STOP_DIFFERENTIAL; break; }
    }
    sweep_result(Pb, Pe, &hb, lc.k, n, it, stop, res);
    if (d_out4) {
        { const icpmi_status s = sweep_deskew(c, B, d_scan, n, d_t_rel, Pb, Pe, opts, d_out4); if (s != ICPMI_OK) return s; }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return ICPMI_OK;
}
