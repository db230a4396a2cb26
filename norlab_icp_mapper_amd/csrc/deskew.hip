// deskew.hip -- sweep deskewing: per-point motion compensation of a scan (include/icpmi.h: icpmi_deskew_table, icpmi_deskew,
// icpmi_deskew_dev; the reference asks its users to switch deskewing on, docs/UsingInRos.md:211-224, and leaves it to the ROS wrapper).
//
// Two halves.  deskew_prepare (host, double precision, no device call) checks the caller's table of timed poses and turns it into what
// the kernel reads: the poses RELATIVE to the pose at the reference time (so translations are the centimetres the sensor moved during
// the sweep, not map coordinates), the quaternions sign-continued from one stamp to the next, and per segment the angle Omega between
// its two quaternions with 1 / sin(Omega) -- computed here from atan2, not on the device from acosf of a number next to 1.  That is
// what makes float32 enough on the device.
//
// deskew_kernel: one thread per point, no atomics, no shared memory.  The table (at most 1024 stamps: 8 KiB of stamps, 16 KiB of
// quaternions, 16 KiB of translations, 8 KiB of segment constants) is read THROUGH THE CACHE, not staged in LDS: a lidar's points come
// nearly time-ordered, so the 64 lanes of a wave share one or two segments and the ten steps of the bisection walk the same few
// lines; staging would make every workgroup of 256 points copy up to 48 KiB it reads 100 bytes of.
//
// The arithmetic of one point (float32 unless marked; nothing is contracted, the library is built with -ffp-contract=off):
//   tau = (double)t_rel[i] * time_unit_s                                        (fp64)
//   NaN: the error flag is raised, nothing is written for the point
//   round_s > 0:  tau = rint(tau / round_s) * round_s                           (fp64, ties to even)
//   tau < s_0 or tau > s_{K-1}:  extrapolate ? tau = the bound : error flag, nothing written
//   k = the largest index in [0, K - 2] with s_k <= tau                         (bisection; tau == s_{K-1} gives k = K - 2, u = 1)
//   u = (float)((tau - s_k) / (s_{k+1} - s_k))                                  (fp64, rounded once)
//   um = 1 - u
//   inv_sin_k == 0 ?  w0 = um, w1 = u  :  w0 = sinf(um * Omega_k) * inv_sin_k,  w1 = sinf(u * Omega_k) * inv_sin_k
//   q_c = w0 * q_k,c + w1 * q_{k+1},c   (c = x, y, z, w; not renormalised)      p_c = um * p_k,c + u * p_{k+1},c   (c = x, y, z)
//   xx = qx qx, yy = qy qy, zz = qz qz, xy = qx qy, xz = qx qz, yz = qy qz, wx = qw qx, wy = qw qy, wz = qw qz
//   R = | 1 - 2 (yy + zz)    2 (xy - wz)        2 (xz + wy)     |
//       | 2 (xy + wz)        1 - 2 (xx + zz)    2 (yz - wx)     |
//       | 2 (xz - wy)        2 (yz + wx)        1 - 2 (xx + yy) |
//   out_r = ((R_r0 x + R_r1 y) + R_r2 z) + p_r;  out_3 = in_3;  normal_r = (R_r0 nx + R_r1 ny) + R_r2 nz
#include "common.h"

#include <cmath>

namespace {

// the device copy of the table, one block: [flag word, 12 bytes of padding][K stamps, double, padded to 16 bytes][K quaternions, float4 (x, y, z, w)]
// [K translations, float4 (x, y, z, 0)][K - 1 segment constants, float2 (Omega, 1 / sin Omega or 0)]
struct DeskewView {
    unsigned* flag;
    const double* stamp;
    const float4* q;
    const float4* p;
    const float2* seg;
    int K;
    int extrapolate;
    double unit, round_s;
};

// in / out and nin / nout may be the same arrays: a thread reads its own point before it writes it
__global__ __launch_bounds__(256) void deskew_kernel(const float4* in, int64_t n, const float* __restrict__ t_rel, DeskewView v, float4* out,
                                                     const float* nin, float* nout)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double tau = (double)t_rel[i] * v.unit;
    if (tau != tau) { *v.flag = 1u; return; }
    if (v.round_s > 0.0) tau = rint(tau / v.round_s) * v.round_s;
    const double s_first = v.stamp[0], s_last = v.stamp[v.K - 1];
    if (tau < s_first || tau > s_last) {
        if (!v.extrapolate) { *v.flag = 1u; return; }
        tau = tau < s_first ? s_first : s_last;
    }
    int lo = 0, hi = v.K - 1; // s_lo <= tau, and tau < s_hi or hi == K - 1
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v.stamp[mid] <= tau) lo = mid; else hi = mid;
    }
    const double s0 = v.stamp[lo], s1 = v.stamp[lo + 1];
    const float u = (float)((tau - s0) / (s1 - s0));
    const float um = 1.0f - u;
    const float2 sg = v.seg[lo];
    float w0 = um, w1 = u;
    if (sg.y != 0.0f) { w0 = sinf(um * sg.x) * sg.y; w1 = sinf(u * sg.x) * sg.y; }
    const float4 qa = v.q[lo], qb = v.q[lo + 1], pa = v.p[lo], pb = v.p[lo + 1];
    const float qx = w0 * qa.x + w1 * qb.x, qy = w0 * qa.y + w1 * qb.y, qz = w0 * qa.z + w1 * qb.z, qw = w0 * qa.w + w1 * qb.w;
    const float px = um * pa.x + u * pb.x, py = um * pa.y + u * pb.y, pz = um * pa.z + u * pb.z;
    const float xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
    const float r00 = 1.0f - 2.0f * (yy + zz), r01 = 2.0f * (xy - wz), r02 = 2.0f * (xz + wy);
    const float r10 = 2.0f * (xy + wz), r11 = 1.0f - 2.0f * (xx + zz), r12 = 2.0f * (yz - wx);
    const float r20 = 2.0f * (xz - wy), r21 = 2.0f * (yz + wx), r22 = 1.0f - 2.0f * (xx + yy);
    const float4 x = in[i];
    float4 o;
    o.x = ((r00 * x.x + r01 * x.y) + r02 * x.z) + px;
    o.y = ((r10 * x.x + r11 * x.y) + r12 * x.z) + py;
    o.z = ((r20 * x.x + r21 * x.y) + r22 * x.z) + pz;
    o.w = x.w;
    out[i] = o;
    if (nin) {
        const float nx = nin[3 * i], ny = nin[3 * i + 1], nz = nin[3 * i + 2];
        nout[3 * i] = (r00 * nx + r01 * ny) + r02 * nz;
        nout[3 * i + 1] = (r10 * nx + r11 * ny) + r12 * nz;
        nout[3 * i + 2] = (r20 * nx + r21 * ny) + r22 * nz;
    }
}

struct Quat { double x, y, z, w; };
inline double qdot(const Quat& a, const Quat& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
inline Quat qscaled(const Quat& a, double s) { return Quat{a.x * s, a.y * s, a.z * s, a.w * s}; }
inline Quat qnormalised(const Quat& a) { return qscaled(a, 1.0 / std::sqrt(qdot(a, a))); }
inline Quat qmul(const Quat& a, const Quat& b) // Hamilton product: the rotation of b, then of a
{
    return Quat{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
                a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
// the angle between two unit quaternions as 4-vectors, exact to rounding for small and for large angles alike
inline double qangle(const Quat& a, const Quat& b)
{
    const Quat d{b.x - a.x, b.y - a.y, b.z - a.z, b.w - a.w}, s{b.x + a.x, b.y + a.y, b.z + a.z, b.w + a.w};
    return 2.0 * std::atan2(std::sqrt(qdot(d, d)), std::sqrt(qdot(s, s)));
}
constexpr double DESKEW_LERP_BELOW = 1.0 / 1048576.0; // 2^-20: below it sin(u Omega) / sin(Omega) is u to float32 precision

struct DeskewTable {
    std::vector<double> stamp;  // K
    std::vector<float> q4, p3;  // 4 K, 3 K
    std::vector<float> omega, inv_sin; // K - 1
};

// checks the caller's motion and builds the float32 table; false with the reason in err
bool deskew_prepare(const icpmi_sweep_motion* m, DeskewTable& t, std::string& err)
{
    if (!m || !m->stamp_s || !m->pose7) { err = "deskew: NULL motion, stamp_s or pose7"; return false; }
    const int K = m->n_poses;
    if (K < 2 || K > ICPMI_DESKEW_MAX_POSES) { err = "deskew: n_poses must be in [2, " + std::to_string((int)ICPMI_DESKEW_MAX_POSES) + "]"; return false; }
    if (!(std::isfinite(m->time_unit_s) && m->time_unit_s > 0.0)) { err = "deskew: time_unit_s must be finite and > 0"; return false; }
    if (!(std::isfinite(m->round_s) && m->round_s >= 0.0)) { err = "deskew: round_s must be finite and >= 0"; return false; }
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(m->stamp_s[k])) { err = "deskew: stamp " + std::to_string(k) + " is not finite"; return false; }
        if (k > 0 && !(m->stamp_s[k] > m->stamp_s[k - 1])) { err = "deskew: stamps must be strictly increasing (stamp " + std::to_string(k) + ")"; return false; }
        const double* P = m->pose7 + 7 * (size_t)k;
        for (int c = 0; c < 7; ++c) if (!std::isfinite(P[c])) { err = "deskew: pose " + std::to_string(k) + " has a non-finite entry"; return false; }
        const double len = std::sqrt(P[3] * P[3] + P[4] * P[4] + P[5] * P[5] + P[6] * P[6]);
        if (!(std::fabs(len - 1.0) <= 1e-3)) { err = "deskew: the quaternion of pose " + std::to_string(k) + " is not of unit length"; return false; }
    }
    if (!(m->ref_s >= m->stamp_s[0] && m->ref_s <= m->stamp_s[K - 1])) { err = "deskew: ref_s lies outside [stamp_s[0], stamp_s[n_poses - 1]]"; return false; }
    const auto quat_of = [&](int k) { const double* P = m->pose7 + 7 * (size_t)k; return qnormalised(Quat{P[3], P[4], P[5], P[6]}); };
    // T(ref_s): translation lerp, rotation slerp along the shorter arc
    int kr = 0;
    while (kr < K - 2 && m->stamp_s[kr + 1] <= m->ref_s) ++kr;
    const double ur = (m->ref_s - m->stamp_s[kr]) / (m->stamp_s[kr + 1] - m->stamp_s[kr]);
    const double* Pa = m->pose7 + 7 * (size_t)kr; const double* Pb = Pa + 7;
    const double pr[3] = {(1.0 - ur) * Pa[0] + ur * Pb[0], (1.0 - ur) * Pa[1] + ur * Pb[1], (1.0 - ur) * Pa[2] + ur * Pb[2]};
    const Quat qa = quat_of(kr);
    Quat qb = quat_of(kr + 1);
    if (qdot(qa, qb) < 0.0) qb = qscaled(qb, -1.0);
    const double om = qangle(qa, qb);
    double w0 = 1.0 - ur, w1 = ur;
    if (om >= DESKEW_LERP_BELOW) { w0 = std::sin((1.0 - ur) * om) / std::sin(om); w1 = std::sin(ur * om) / std::sin(om); }
    const Quat qr = qnormalised(Quat{w0 * qa.x + w1 * qb.x, w0 * qa.y + w1 * qb.y, w0 * qa.z + w1 * qb.z, w0 * qa.w + w1 * qb.w});
    const Quat qri{-qr.x, -qr.y, -qr.z, qr.w};
    // the rows of R(ref)^T are the columns of R(ref)
    const double xx = qr.x * qr.x, yy = qr.y * qr.y, zz = qr.z * qr.z, xy = qr.x * qr.y, xz = qr.x * qr.z, yz = qr.y * qr.z, wx = qr.w * qr.x,
                 wy = qr.w * qr.y, wz = qr.w * qr.z;
    const double R[3][3] = {{1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)},
                            {2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)},
                            {2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)}};
    t.stamp.assign(m->stamp_s, m->stamp_s + K);
    t.q4.resize(4 * (size_t)K); t.p3.resize(3 * (size_t)K); t.omega.resize((size_t)K - 1); t.inv_sin.resize((size_t)K - 1);
    Quat prev{0, 0, 0, 1};
    for (int k = 0; k < K; ++k) {
        const double* P = m->pose7 + 7 * (size_t)k;
        Quat q = qnormalised(qmul(qri, quat_of(k)));   // T(ref)^-1 T_k
        if (k > 0 && qdot(prev, q) < 0.0) q = qscaled(q, -1.0);
        const double d[3] = {P[0] - pr[0], P[1] - pr[1], P[2] - pr[2]};
        for (int c = 0; c < 3; ++c) t.p3[3 * (size_t)k + c] = (float)(R[0][c] * d[0] + R[1][c] * d[1] + R[2][c] * d[2]);
        t.q4[4 * (size_t)k] = (float)q.x; t.q4[4 * (size_t)k + 1] = (float)q.y; t.q4[4 * (size_t)k + 2] = (float)q.z; t.q4[4 * (size_t)k + 3] = (float)q.w;
        if (k > 0) {
            const double o = qangle(prev, q);
            t.omega[(size_t)k - 1] = (float)o;
            t.inv_sin[(size_t)k - 1] = o < DESKEW_LERP_BELOW ? 0.0f : (float)(1.0 / std::sin(o));
        }
        prev = q;
    }
    return true;
}

// the table as one block (layout: DeskewView), the cleared flag word in front: one upload
struct DeskewBlob { std::vector<unsigned char> bytes; size_t off_stamp, off_q, off_p, off_seg; };
DeskewBlob deskew_blob(const DeskewTable& t, int K)
{
    DeskewBlob b;
    b.off_stamp = 16; b.off_q = (b.off_stamp + sizeof(double) * (size_t)K + 15) & ~(size_t)15; b.off_p = b.off_q + sizeof(float4) * (size_t)K;
    b.off_seg = b.off_p + sizeof(float4) * (size_t)K;
    b.bytes.assign(b.off_seg + sizeof(float2) * (size_t)(K - 1), 0);
    memcpy(b.bytes.data() + b.off_stamp, t.stamp.data(), sizeof(double) * (size_t)K);
    float* bq = (float*)(b.bytes.data() + b.off_q); float* bp = (float*)(b.bytes.data() + b.off_p); float* bs = (float*)(b.bytes.data() + b.off_seg);
    for (int k = 0; k < K; ++k) {
        for (int r = 0; r < 4; ++r) bq[4 * k + r] = t.q4[4 * (size_t)k + r];
        for (int r = 0; r < 3; ++r) bp[4 * k + r] = t.p3[3 * (size_t)k + r];
        if (k < K - 1) { bs[2 * k] = t.omega[(size_t)k]; bs[2 * k + 1] = t.inv_sin[(size_t)k]; }
    }
    return b;
}
// ... and the kernel's view of its device copy
DeskewView deskew_view(unsigned char* d_tab, const DeskewBlob& b, const icpmi_sweep_motion* m)
{
    DeskewView v;
    v.flag = (unsigned*)d_tab; v.stamp = (const double*)(d_tab + b.off_stamp); v.q = (const float4*)(d_tab + b.off_q);
    v.p = (const float4*)(d_tab + b.off_p); v.seg = (const float2*)(d_tab + b.off_seg);
    v.K = m->n_poses; v.extrapolate = m->extrapolate ? 1 : 0; v.unit = m->time_unit_s; v.round_s = m->round_s;
    return v;
}

} // namespace

// deskew_kernel on device pointers WITHOUT the wait for its error flag: for a caller that has checked the point times itself and set
// extrapolate, so that no point can raise the flag (sweep.hip: every iteration of a sweep registration deskews the raw scan again).
// d_tab: the caller's block for the table, at least ICPMI_UP_SLOT bytes, not reused before the kernel has run.  The table travels
// through one slot of the pinned upload ring, so it must fit one (a two-pose table is 104 bytes).  d_out != d_in.
icpmi_status deskew_enqueue_dev(icpmi_ctx* c, const float4* d_in, int64_t n, const float* d_t_rel, const icpmi_sweep_motion* m, unsigned char* d_tab,
                                float4* d_out)
{
    DeskewTable t;
    if (!deskew_prepare(m, t, c->last_error)) return ICPMI_ERR_INVALID_ARG;
    if (n == 0) return ICPMI_OK;
    const DeskewBlob b = deskew_blob(t, m->n_poses);
    if (b.bytes.size() > ICPMI_UP_SLOT) { c->last_error = "deskew: the table does not fit one upload slot"; return ICPMI_ERR_UNSUPPORTED; }
    { const icpmi_status us = upload_small(c, d_tab, b.bytes.data(), b.bytes.size()); if (us != ICPMI_OK) return us; }
    if (!c->h_pin) HIP_TRY(c, hipStreamSynchronize(c->stream)); // (no pinned ring: the copy read `b` itself)
    hipLaunchKernelGGL(deskew_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_in, n, d_t_rel, deskew_view(d_tab, b, m), d_out,
                       (const float*)nullptr, (float*)nullptr);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// icpmi_deskew_table: no handle, no device call
icpmi_status deskew_table_host(const icpmi_sweep_motion* m, float* q4, float* p3, float* omega, float* inv_sin, std::string& err)
{
    if (!q4 || !p3 || !omega || !inv_sin) { err = "deskew_table: a NULL output"; return ICPMI_ERR_INVALID_ARG; }
    DeskewTable t;
    if (!deskew_prepare(m, t, err)) return ICPMI_ERR_INVALID_ARG;
    std::copy(t.q4.begin(), t.q4.end(), q4);
    std::copy(t.p3.begin(), t.p3.end(), p3);
    std::copy(t.omega.begin(), t.omega.end(), omega);
    std::copy(t.inv_sin.begin(), t.inv_sin.end(), inv_sin);
    return ICPMI_OK;
}

// icpmi_deskew (dev == false: host pointers, staged on the handle) and icpmi_deskew_dev (dev == true: device pointers on the handle's
// stream, out4 == in4 and out_normals3 == in_normals3 allowed).  The pointers are checked by the callers in api.hip.
icpmi_status ops_deskew(icpmi_ctx* c, const float* in4, int64_t n, const float* t_rel, const icpmi_sweep_motion* m, float* out4,
                        const float* in_normals3, float* out_normals3, bool dev)
{
    DeskewTable t;
    if (!deskew_prepare(m, t, c->last_error)) return ICPMI_ERR_INVALID_ARG;
    const int K = m->n_poses;
    if (c->cfg.is_2d) {
        for (int k = 0; k < K; ++k) {
            const double* P = m->pose7 + 7 * (size_t)k;
            if (P[2] != 0.0 || P[3] != 0.0 || P[4] != 0.0) {
                c->last_error = "deskew: a planar (2-D) handle takes planar motion only: tz, qx and qy of every pose must be exactly 0"; return ICPMI_ERR_INVALID_ARG;
            }
        }
    }
    if (n == 0) return ICPMI_OK;
    if (n > 0x7fffffffll) { c->last_error = "deskew: more than 2^31 - 1 points"; return ICPMI_ERR_UNSUPPORTED; }
    const DeskewBlob b = deskew_blob(t, K);
    const std::vector<unsigned char>& blob = b.bytes;
    const size_t bytes = blob.size();
    // every block first: nothing below gives up between an upload from `blob` and the wait at the flag's read-back
    unsigned char* d_tab = scratch_get<unsigned char>(c, 17, bytes);
    if (!d_tab) return ICPMI_ERR_HIP;
    float* d_ts = nullptr;
    if (!dev) {
        if (c->d_stage_in.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        if (in_normals3 && c->d_stage_n3.ensure(c, (size_t)n * 3) != ICPMI_OK) return ICPMI_ERR_HIP;
        if (!(d_ts = scratch_get<float>(c, 18, (size_t)n))) return ICPMI_ERR_HIP;
    }
    { const icpmi_status us = upload_small(c, d_tab, blob.data(), bytes); if (us != ICPMI_OK) return us; }
    const DeskewView v = deskew_view(d_tab, b, m);
    const float4* d_in = (const float4*)in4; float4* d_out = (float4*)out4;
    const float* d_t = t_rel; const float* d_nin = in_normals3; float* d_nout = out_normals3;
    if (!dev) { // staged on the handle, deskewed in place there
        HIP_TRY(c, hipMemcpyAsync(c->d_stage_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_ts, t_rel, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        d_in = c->d_stage_in; d_out = c->d_stage_in; d_t = d_ts;
        if (in_normals3) {
            HIP_TRY(c, hipMemcpyAsync(c->d_stage_n3, in_normals3, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
            d_nin = c->d_stage_n3; d_nout = c->d_stage_n3;
        }
    }
    hipLaunchKernelGGL(deskew_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_in, n, d_t, v, d_out, d_nin, d_nout);
    HIP_TRY(c, hipGetLastError());
    unsigned flag = 0;
    if (read_back(c, &flag, v.flag, sizeof flag) != ICPMI_OK) return ICPMI_ERR_HIP; // (waits for the kernel: `blob` and the caller's arrays are free)
    if (flag) {
        c->last_error = m->extrapolate ? "deskew: a point time is NaN"
                                       : "deskew: a point time is NaN or lies outside [stamp_s[0], stamp_s[n_poses - 1]] (ExtrapolationException)";
        return ICPMI_ERR_INVALID_ARG;
    }
    if (!dev) {
        HIP_TRY(c, hipMemcpyAsync(out4, d_out, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        if (in_normals3) HIP_TRY(c, hipMemcpyAsync(out_normals3, d_nout, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return ICPMI_OK;
}
