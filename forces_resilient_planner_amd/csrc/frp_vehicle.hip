// frp_vehicle.hip -- frp_nmpc.h section (12), frp_nmpc_vehicle.h: the vehicle that flies the command timer's samples (a controller with no
// reference counterpart around the planner's own dynamics, frp_model.hpp's accel) and NMPCManage's two odometry callbacks
// (plan_manage/src/nmpc_manage.cpp:421-478) with the message producer that feeds them.
//
//   * One thread per vehicle, 256 per workgroup, no LDS, no barrier, no atomics: a vehicle reads and writes its own rows alone.  The nine
//     states, the hold and the gains live in registers across the S samples; per sample a thread reads one 128-byte command row and its
//     kind, and (where asked) writes 72 bytes of trace.  Rows of neighbouring lanes are S * 128 bytes apart, so the loads are not
//     coalesced -- at 4096 vehicles and S = 5 that is 2.6 MB per call against a launch of a few microseconds: the cost is the launch and
//     the serial chain of S * n_sub Heun steps (two accelerations each; the second stage's sines and cosines are the next step's first:
//     the angles are the same doubles, so they are computed once).
//   * The plant is frp_model.hpp's accel_t<false> with make_trig, i.e. accel() with that reuse: not re-derived here.  Bounds are that
//     file's lower_bound / upper_bound.
//   * No contraction in this file (the build passes -ffp-contract=off as well): every product and sum of the controller and of the Heun
//     update is rounded on its own, as tests/vehicle_oracle.py writes them; the model's sincos_bounded carries explicit fma calls, which
//     stay.  sqrt and the divisions are IEEE; asin, atan2 and ceil are ocml's.
//   * Every index is b < B and s < S as the entry point checked them (B * S fits an int; offsets are formed in size_t).
//   * Every store is a plain C++ store from a vector lane; no inline assembly.
//   * frp_nmpc_vehicle_step_observed (frp_nmpc_estimator.h) is the same step kernel instantiated with one more store per sample, the
//     clamped thrust; the instantiation frp_nmpc_vehicle_step launches is the kernel as it was (profiles/estimator_step_identity.txt).
//   * frp_nmpc_vehicle_step_field (frp_nmpc.h section 15) is the same step kernel with FIELD set: between a sample's setpoint and its
//     controller the force is taken from frp_disturbance.hpp's sample_force at the plant's own position, and replaces f for the sample's
//     Heun steps.  The two instantiations without FIELD are the kernels as they were (profiles/disturbance_step_identity.txt).  The
//     constant part and the OU state are re-read from memory per sample, not held across the Heun steps: the kernel sits at 230 VGPRs,
//     and twelve more registers of live state would spill.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_model.hpp"
#include "frp_disturbance.hpp"
#include "frp_fleet.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace vehicle {

using namespace fleet;

constexpr int NXV = FRP_VEHICLE_STATE, HOLD = FRP_VEHICLE_HOLD_STRIDE, MSG = FRP_VEHICLE_MSG_STRIDE, CMD = FRP_COMMAND_STRIDE;

__device__ inline double clampd(double v, double lo, double hi, int *which)
{
    *which = v < lo ? -1 : v > hi ? 1 : 0;
    return v < lo ? lo : v > hi ? hi : v;
}

// OBSERVED: frp_nmpc_vehicle_step_observed's instantiation (frp_nmpc_estimator.h) also stores the clamped thrust of every sample;
// frp_nmpc_vehicle_step launches <false>, whose code has no such store (`thrust` is then not read).
// FIELD: frp_nmpc_vehicle_step_field's instantiations take every sample's force from the disturbance model d (c.f_true is its constant
// part) and store it to `force` where asked; without FIELD neither d nor force is read.
template <bool OBSERVED, bool FIELD>
__global__ __launch_bounds__(THREADS) void step_kernel(frp_nmpc_vehicle c, double *thrust, frp_nmpc_disturbance d, double *force)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= c.B) return;
    const int S = c.S, n_sub = c.n_sub;
    double x[NXV], hp[3], hyaw, f[3];
#pragma unroll
    for (int i = 0; i < NXV; i++) x[i] = c.x[(size_t)b * NXV + i];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        hp[i] = c.hold[(size_t)b * HOLD + i];
        f[i] = c.f_true[(size_t)b * 3 + i];
    }
    hyaw = c.hold[(size_t)b * HOLD + 3];
    const double h = c.dt_cmd / (double)n_sub;
    const double t_lo = lower_bound(3), t_hi = upper_bound(3), a_lo = lower_bound(14), a_hi = upper_bound(14);
    Trig tg = make_trig(x + 6);
    for (int s = 0; s < S; s++) {
        // ---- the setpoint ----
        const double *row = c.cmd + ((size_t)b * S + s) * CMD;
        const int kind = c.kind[(size_t)b * S + s];
        double p_ref[3], v_ref[3] = {0.0, 0.0, 0.0}, w_ff[3] = {0.0, 0.0, 0.0}, a_ff[3] = {0.0, 0.0, 0.0}, yaw;
        if (kind == FRP_COMMAND_TRAJ || kind == FRP_COMMAND_END || kind == FRP_COMMAND_YAW) {
#pragma unroll
            for (int i = 0; i < 3; i++) p_ref[i] = row[i];
            if (kind == FRP_COMMAND_YAW) {
                yaw = row[12];
            } else {
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    v_ref[i] = row[7 + i];
                    w_ff[i] = row[10 + i];
                    a_ff[i] = row[13 + i];
                }
                const double qx = row[3], qy = row[4], qz = row[5], qw = row[6];
                const double ty = 2.0 * qy, tz = 2.0 * qz;
                const double twz = tz * qw, txy = ty * qx, tyy = ty * qy, tzz = tz * qz;
                yaw = atan2(-(txy - twz), 1.0 - (tyy + tzz));
            }
#pragma unroll
            for (int i = 0; i < 3; i++) hp[i] = p_ref[i];
            hyaw = yaw;
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) p_ref[i] = hp[i];
            yaw = hyaw;
        }
        if (FIELD) { // ---- the force this sample flies under: the model at the position before the sample ----
            double base[3], g[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < 3; i++) base[i] = c.f_true[(size_t)b * 3 + i];
            if (d.gust) {
#pragma unroll
                for (int i = 0; i < 3; i++) g[i] = d.gust[(size_t)b * 3 + i];
            }
            const long long k = d.tick[b];
            disturbance::sample_force(d, d.zone, d.event, b, k, x, base, g, f);
            if (d.gust) {
#pragma unroll
                for (int i = 0; i < 3; i++) d.gust[(size_t)b * 3 + i] = g[i];
            }
            d.tick[b] = (long long)((unsigned long long)k + 1ULL);
            if (force) {
#pragma unroll
                for (int i = 0; i < 3; i++) force[((size_t)b * S + s) * 3 + i] = f[i];
            }
        }
        // ---- the controller ----
        int sat = 0, which;
        double a[3];
#pragma unroll
        for (int i = 0; i < 3; i++) a[i] = a_ff[i] + c.kp[i] * (p_ref[i] - x[i]) + c.kv[i] * (v_ref[i] - x[3 + i]);
        a[2] = a[2] + c.g;
        const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double T = clampd(c.mass * na, t_lo, t_hi, &which);
        sat |= which < 0 ? FRP_VEHICLE_SAT_THRUST_LO : which > 0 ? FRP_VEHICLE_SAT_THRUST_HI : 0;
        double zb[3] = {0.0, 0.0, 1.0};
        if (na == 0.0) {
            sat |= FRP_VEHICLE_SAT_ZERO_ACC;
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) zb[i] = a[i] / na;
        }
        double sy, cy;
        sincos_bounded(yaw, &sy, &cy);
        const double cx = cy * zb[0] + sy * zb[1];
        const double cyy = cy * zb[1] - sy * zb[0];
        const double sr = clampd(-cyy, -1.0, 1.0, &which);
        const double roll = clampd(asin(sr), a_lo, a_hi, &which);
        sat |= which ? FRP_VEHICLE_SAT_ROLL : 0;
        const double pitch = clampd(atan2(cx, zb[2]), a_lo, a_hi, &which);
        sat |= which ? FRP_VEHICLE_SAT_PITCH : 0;
        const double d = yaw - x[8];
        const double k = ceil((d - PI) / (2.0 * PI));
        sat |= k != 0.0 ? FRP_VEHICLE_SAT_YAW_WRAP : 0;
        const double err[3] = {roll - x[6], pitch - x[7], d - 2.0 * PI * k};
        double w[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            w[i] = clampd(w_ff[i] + c.ka[i] * err[i], lower_bound(i), upper_bound(i), &which);
            sat |= which ? (FRP_VEHICLE_SAT_RATE0 << i) : 0;
        }
        // ---- the plant: n_sub Heun steps with (w, T) held ----
        for (int n = 0; n < n_sub; n++) {
            double a1[3], a2[3], vt[3], et[3];
            accel_t<false>(x + 3, tg, T, f, a1, nullptr);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                vt[i] = x[3 + i] + h * a1[i];
                et[i] = x[6 + i] + h * w[i];
            }
            tg = make_trig(et); // (the next step's first stage evaluates the same angles)
            accel_t<false>(vt, tg, T, f, a2, nullptr);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                x[i] = x[i] + 0.5 * h * (x[3 + i] + vt[i]);
                x[3 + i] = x[3 + i] + 0.5 * h * (a1[i] + a2[i]);
                x[6 + i] = et[i];
            }
        }
        if (c.trace) {
#pragma unroll
            for (int i = 0; i < NXV; i++) c.trace[((size_t)b * S + s) * NXV + i] = x[i];
        }
        if (c.sat) c.sat[(size_t)b * S + s] = sat;
        if (OBSERVED) thrust[(size_t)b * S + s] = T;
    }
#pragma unroll
    for (int i = 0; i < NXV; i++) c.x[(size_t)b * NXV + i] = x[i];
    double *ho = c.hold + (size_t)b * HOLD;
    ho[0] = hp[0]; ho[1] = hp[1]; ho[2] = hp[2]; ho[3] = hyaw;
    ho[4] = 0.0; ho[5] = 0.0; ho[6] = 0.0; ho[7] = 0.0;
}

__global__ __launch_bounds__(THREADS) void reset_kernel(int B, const double *x0, const int *mask, double *x, double *hold)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    if (mask && mask[b] == 0) return;
    const double *s = x0 + (size_t)b * NXV;
    double *d = x + (size_t)b * NXV, *ho = hold + (size_t)b * HOLD;
#pragma unroll
    for (int i = 0; i < NXV; i++) d[i] = s[i];
    ho[0] = s[0]; ho[1] = s[1]; ho[2] = s[2]; ho[3] = s[8];
    ho[4] = 0.0; ho[5] = 0.0; ho[6] = 0.0; ho[7] = 0.0;
}

// eulerToRot's qz * qy * qx (nmpc_solver.cpp:554-564)
__device__ inline Quat euler_quaternion(const double *e)
{
    double sr, cr, sp, cp, sy, cy;
    sincos_bounded(0.5 * e[0], &sr, &cr);
    sincos_bounded(0.5 * e[1], &sp, &cp);
    sincos_bounded(0.5 * e[2], &sy, &cy);
    const Quat qx = {cr, sr, 0.0, 0.0}, qy = {cp, 0.0, sp, 0.0}, qz = {cy, 0.0, 0.0, sy};
    return qmul(qmul(qz, qy), qx);
}

__global__ __launch_bounds__(THREADS) void message_kernel(int B, int type, const double *x, double *msg)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    const double *s = x + (size_t)b * NXV;
    double *m = msg + (size_t)b * MSG;
    const Quat q = euler_quaternion(s + 6);
    double v[3] = {s[3], s[4], s[5]};
    if (type == FRP_ODOM_BODY) {
        double R[9];
        rotation(q, R);
        const double v0 = v[0], v1 = v[1], v2 = v[2];
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = R[i] * v0 + R[3 + i] * v1 + R[6 + i] * v2; // R' v
    }
    m[0] = s[0]; m[1] = s[1]; m[2] = s[2];
    m[3] = q.x; m[4] = q.y; m[5] = q.z; m[6] = q.w;
    m[7] = v[0]; m[8] = v[1]; m[9] = v[2];
    m[10] = 0.0; m[11] = 0.0; m[12] = 0.0;
}

// nmpc_manage.cpp:421-448 (FRP_ODOM_WORLD), :456-478 (FRP_ODOM_BODY)
__global__ __launch_bounds__(THREADS) void odometry_kernel(int B, int type, const double *msg, const int *fresh, double *state, double *state_prev, int *have_odom)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    if (fresh[b] == 0) return;
    const double *m = msg + (size_t)b * MSG;
    double *st = state + (size_t)b * NXV;
    if (state_prev) { // :427, :461
#pragma unroll
        for (int i = 0; i < NXV; i++) state_prev[(size_t)b * NXV + i] = st[i];
    }
    const Quat q = {m[6], m[3], m[4], m[5]};
    double v[3] = {m[7], m[8], m[9]};
    if (type == FRP_ODOM_BODY) { // :468-469
        double R[9];
        rotation(q, R);
        const double v0 = v[0], v1 = v[1], v2 = v[2];
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = R[3 * i] * v0 + R[3 * i + 1] * v1 + R[3 * i + 2] * v2;
    }
    st[0] = m[0]; st[1] = m[1]; st[2] = m[2];
    st[3] = v[0]; st[4] = v[1]; st[5] = v[2];
    // mav_msgs::getEulerAnglesFromQuaternion
    st[6] = atan2(2.0 * (q.w * q.x + q.y * q.z), 1.0 - 2.0 * (q.x * q.x + q.y * q.y));
    st[7] = asin(2.0 * (q.w * q.y - q.z * q.x));
    st[8] = atan2(2.0 * (q.w * q.z + q.x * q.y), 1.0 - 2.0 * (q.y * q.y + q.z * q.z));
    have_odom[b] = 1; // :447, :477
}

} // namespace vehicle
} // namespace frp

extern "C" {

// the argument rules of frp_nmpc_vehicle_step and of frp_nmpc_vehicle_step_observed
static int step_args(const frp_nmpc_vehicle *v)
{
    using namespace frp::vehicle;
    if (!v || v->B < 1 || v->S < 1 || (long long)v->B * v->S > 0x7fffffffLL || v->n_sub < 1 || v->n_sub > FRP_VEHICLE_MAX_SUB) return FRP_ERR_ARG;
    if (!positive(v->mass) || !positive(v->dt_cmd) || !finite_d(v->g)) return FRP_ERR_ARG;
    for (int i = 0; i < 3; i++)
        if (!non_negative(v->kp[i]) || !non_negative(v->kv[i]) || !non_negative(v->ka[i])) return FRP_ERR_ARG;
    if (!v->x || !v->f_true || !v->cmd || !v->kind || !v->hold) return FRP_ERR_ARG;
    return FRP_OK;
}

int frp_nmpc_vehicle_step(const frp_nmpc_vehicle *v, void *stream)
{
    using namespace frp::vehicle;
    if (step_args(v) != FRP_OK) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(step_kernel<false, false>, blocks_for(v->B), stream, *v, nullptr, frp_nmpc_disturbance{}, nullptr);
}

// frp_nmpc_estimator.h
int frp_nmpc_vehicle_step_observed(const frp_nmpc_vehicle *v, double *thrust, void *stream)
{
    using namespace frp::vehicle;
    if (step_args(v) != FRP_OK || !thrust) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(step_kernel<true, false>, blocks_for(v->B), stream, *v, thrust, frp_nmpc_disturbance{}, nullptr);
}

// frp_nmpc.h section (15)
int frp_nmpc_vehicle_step_field(const frp_nmpc_vehicle *v, const frp_nmpc_disturbance *d, double *thrust, double *force, void *stream)
{
    using namespace frp::vehicle;
    if (step_args(v) != FRP_OK || frp::disturbance::check(d) != FRP_OK || d->B != v->B || !(d->dt == v->dt_cmd)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(thrust ? step_kernel<true, true> : step_kernel<false, true>, blocks_for(v->B), stream, *v, thrust, *d, force);
}

int frp_nmpc_vehicle_reset(int B, const double *x0, const int *mask, double *x, double *hold, void *stream)
{
    using namespace frp::vehicle;
    if (B < 1 || !x0 || !x || !hold) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(reset_kernel, blocks_for(B), stream, B, x0, mask, x, hold);
}

int frp_nmpc_vehicle_message(int B, int type, const double *x, double *msg, void *stream)
{
    using namespace frp::vehicle;
    if (B < 1 || (type != FRP_ODOM_WORLD && type != FRP_ODOM_BODY) || !x || !msg) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(message_kernel, blocks_for(B), stream, B, type, x, msg);
}

int frp_nmpc_vehicle_odometry(int B, int type, const double *msg, const int *fresh, double *state, double *state_prev, int *have_odom, void *stream)
{
    using namespace frp::vehicle;
    if (B < 1 || (type != FRP_ODOM_WORLD && type != FRP_ODOM_BODY) || !msg || !fresh || !state || !have_odom) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(odometry_kernel, blocks_for(B), stream, B, type, msg, fresh, state, state_prev, have_odom);
}

} // extern "C"
