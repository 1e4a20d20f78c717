// frp_command.hip -- frp_nmpc.h section (9), frp_nmpc_command.h: NMPCSolver::cmdTrajCallback (plan_manage/src/nmpc_solver.cpp:865-987),
// the 100 Hz timer that samples the last accepted plan and walks cmd_status_, for S consecutive callbacks of B planners in one
// launch; and the snapshot pre_mpc_output_ = mpc_output_ (:527-528) it samples from.
//
//   * A workgroup owns max(1, 256 / S) WHOLE planners, so that status -- read and written in place -- is touched by one workgroup.
//     Phase 1, one thread per planner: the serial part, S steps of the five-state machine.  A step needs one comparison of t_cur at
//     most; it writes kind[b][s] and, after the last step, status / finish / reset_output.  Phase 2, one thread per planner-sample,
//     after a workgroup barrier: what callback s published depends on kind[b][s] and the inputs alone, never on the status, so the
//     samples are independent -- two 136-byte plan rows in, 128 bytes out, a handful of sin / cos.  Bandwidth-trivial: the cost is
//     one launch.
//   * The plan test and the sampled row are frp_fleet.hpp's in_plan and plan_row, the host's operations, one rounding each: no
//     contraction in this file (the build passes -ffp-contract=off as well).  The interpolated slots are therefore the host's bits;
//     sin / cos are ocml's, within an ulp or two of libm's.
//   * The quaternion product and the thrust column of Quaternion::toRotationMatrix are that header's too: Eigen's scalar expressions.
//   * no atomics, no waiting between workgroups, no inline assembly; every store is a plain C++ store from a vector lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_fleet.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace command {

using namespace fleet;

constexpr double REF_PI = 3.1415926; // the file's own constant (nmpc_solver.cpp:3)

// Eigen::Quaternion(AngleAxis(angle, unit axis k)) (Geometry/Quaternion.h: ha = 0.5 * angle; w = cos(ha); vec = sin(ha) * axis) -- and
// eulerToRot's Quaternion(cos(a / 2), .. sin(a / 2) ..) (:558-560): 0.5 * a and a / 2 are the same double, so the two products below
// share their three half-angle sines and cosines
__device__ inline Quat axis_quat(double c, double s, int k)
{
    Quat q;
    q.w = c; q.x = k == 0 ? s : 0.0; q.y = k == 1 ? s : 0.0; q.z = k == 2 ? s : 0.0;
    return q;
}

// eulerToRot(euler) * (0, 0, thrust) (:554-564, :926-927): Matrix3d(qz * qy * qx) times the body thrust
__device__ inline void thrust_world(const Quat &qx, const Quat &qy, const Quat &qz, double thrust, double *out)
{
    thrust_column(qmul(qmul(qz, qy), qx), thrust, out);
}

// sin and cos of a / 2.  Not inlined: ocml's argument reduction holds its constants in scalar registers, and one copy called three times
// keeps the kernel, which already holds the argument struct's 13 pointers there, inside the scalar file without spilling
struct SinCos {
    double s, c;
};
__device__ __noinline__ SinCos sincos_half(double a)
{
    SinCos r;
    const double ha = 0.5 * a;
    r.s = sin(ha); r.c = cos(ha);
    return r;
}

__global__ __launch_bounds__(THREADS) void command_kernel(frp_nmpc_command c, int planners_per_block)
{
    const size_t b0 = (size_t)blockIdx.x * planners_per_block;
    const int S = c.S;
    // ---- phase 1: the state machine (:876-986), one thread per planner ----
    for (int p = threadIdx.x; p < planners_per_block; p += THREADS) {
        const size_t b = b0 + p;
        if (b >= (size_t)c.B) break;
        int st = c.status[b];
        const int have = c.have_traj[b], pub_end = c.pub_end[b];
        int fin = 0;
        bool fin_set = false, reset = false;
        for (int s = 0; s < S; s++) {
            int k = FRP_COMMAND_NONE; // INIT_POSITION, WAIT, anything else: break (:878-881, :895-898)
            if (st == FRP_CMD_ROTATE_YAW) {
                k = c.odom ? FRP_COMMAND_YAW : FRP_COMMAND_NO_YAW_INPUT;
            } else if (st == FRP_CMD_PUB_TRAJ) {
                if (have) { // :903
                    if (in_plan(c.t_cur[b * S + s], c.Ts, c.N)) {
                        k = FRP_COMMAND_TRAJ; fin = 0; // :946
                    } else {
                        fin = 1; // :950
                        if (pub_end) st = FRP_CMD_PUB_END; // :951
                    }
                    fin_set = true;
                }
            } else if (st == FRP_CMD_PUB_END) {
                k = FRP_COMMAND_END; st = FRP_CMD_WAIT; reset = true; // :981, :983
            }
            c.kind[b * S + s] = k;
        }
        c.status[b] = st;
        if (fin_set) c.finish[b] = fin;
        if (reset) c.reset_output[b] = 1;
    }
    __syncthreads(); // (a workgroup-scope fence too: the kind entries below were written by this workgroup)
    // ---- phase 2: what each callback published, one thread per planner-sample ----
    const int total = planners_per_block * S; // <= max(256, S)
    for (int i = threadIdx.x; i < total; i += THREADS) {
        const int p = i / S, s = i - p * S;
        const size_t b = b0 + p;
        if (b >= (size_t)c.B) break;
        const int k = c.kind[b * S + s];
        double o[FRP_COMMAND_STRIDE];
#pragma unroll
        for (int j = 0; j < FRP_COMMAND_STRIDE; j++) o[j] = 0.0;
        double roll = 0.0, pitch = 0.0, yaw = 0.0, thrust = 0.0; // the attitude every published sample carries
        if (k == FRP_COMMAND_TRAJ) { // :905-945
            double q[ROW]; // mpcq (:911); 0 <= t / Ts < N - 1: phase 1 made the test
            const double t = c.t_cur[b * S + s];
            plan_row(c.pre_plan, b * c.N, plan_stage(t, c.Ts), plan_fraction(t, c.Ts), q);
            o[0] = q[8]; o[1] = q[9]; o[2] = q[10];       // :913-915
            o[7] = q[11]; o[8] = q[12]; o[9] = q[13];     // :917-919
            o[10] = q[0]; o[11] = q[1]; o[12] = q[2];     // :921-923
            roll = q[14]; pitch = q[15]; yaw = q[16]; thrust = q[3]; // :925-926
        } else if (k == FRP_COMMAND_END) { // :959-969
            const double *e = c.end_pt + 3 * b, *last = c.pre_plan + (b * c.N + (c.N - 1)) * ROW; // .at(19) for N = 20
            o[0] = e[0]; o[1] = e[1]; o[2] = e[2];
            roll = last[14]; pitch = last[15]; yaw = last[16];
        } else if (k == FRP_COMMAND_YAW) { // :885-889 with callInitYaw's rate (:237-257)
            const double *od = c.odom + 9 * b;
            const double init_yaw = c.init_yaw[b], d = init_yaw - od[8];
            double dot = d;
            if (dot > REF_PI) dot = 2 * REF_PI - dot;        // :239-242, as written
            else if (dot < -REF_PI) dot = dot + 2 * REF_PI;  // :243-246
            const double max_dot = 0.4 * REF_PI;             // :248
            if (dot > max_dot) dot = max_dot;
            else if (dot < -max_dot) dot = -max_dot;
            const double yaw_temp = od[8] + c.t_yaw[b * S + s] * dot;
            // std::min(a, b) = (b < a) ? b : a, std::max(a, b) = (a < b) ? b : a (:886)
            yaw = d >= 0 ? (init_yaw < yaw_temp ? init_yaw : yaw_temp) : (yaw_temp < init_yaw ? init_yaw : yaw_temp);
            o[0] = od[0]; o[1] = od[1]; o[2] = od[2];        // :888
            o[12] = yaw;
        }
        if (k > FRP_COMMAND_NONE) {
            // AngleAxis(roll, X) * AngleAxis(pitch, Y) * AngleAxis(yaw, Z) (:933, :971).  With roll = pitch = 0 the first two factors are
            // exactly (1, 0, 0, 0) and the product is exactly (0, 0, sin(yaw / 2), cos(yaw / 2)): the position + yaw sample
            double sn[3], cs[3];
#pragma nounroll
            for (int a = 0; a < 3; a++) { // (selects, no indexed registers)
                const SinCos r = sincos_half(a == 0 ? roll : a == 1 ? pitch : yaw);
                if (a == 0) { sn[0] = r.s; cs[0] = r.c; }
                if (a == 1) { sn[1] = r.s; cs[1] = r.c; }
                if (a == 2) { sn[2] = r.s; cs[2] = r.c; }
            }
            const Quat qx = axis_quat(cs[0], sn[0], 0), qy = axis_quat(cs[1], sn[1], 1), qz = axis_quat(cs[2], sn[2], 2);
            const Quat q = qmul(qmul(qx, qy), qz);
            o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;  // :935-938
            if (k == FRP_COMMAND_TRAJ) {
                double tw[3];
                thrust_world(qx, qy, qz, thrust, tw);         // :927
                o[13] = tw[0] / c.mass; o[14] = tw[1] / c.mass; o[15] = tw[2] / c.mass - c.g; // :929-931
            }
        }
        double *out = c.cmd + (b * S + s) * FRP_COMMAND_STRIDE;
#pragma unroll
        for (int j = 0; j < FRP_COMMAND_STRIDE; j++) out[j] = o[j];
    }
}

// pre_mpc_output_ = mpc_output_; have_mpc_traj_ = true (:527-528) where accept[b] != 0: one thread per double
__global__ __launch_bounds__(THREADS) void snapshot_kernel(int B, int N, const double *z, const int *accept, double *pre_plan, int *have_traj)
{
    const size_t per = (size_t)N * ROW, i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (size_t)B * per) return;
    const size_t b = i / per;
    if (accept[b] == 0) return;
    pre_plan[i] = z[i];
    if (i == b * per) have_traj[b] = 1;
}

} // namespace command
} // namespace frp

extern "C" {

int frp_nmpc_command_snapshot(int B, int N, const double *z, const int *accept, double *pre_plan, int *have_traj, void *stream)
{
    using namespace frp::command;
    if (B < 1 || N < 2 || N > 64 || !z || !accept || !pre_plan || !have_traj) return FRP_ERR_ARG;
    const size_t blocks = ((size_t)B * N * ROW + THREADS - 1) / THREADS;
    if (blocks > 0x7fffffffu) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(snapshot_kernel, (unsigned)blocks, stream, B, N, z, accept, pre_plan, have_traj);
}

int frp_nmpc_command_batch(const frp_nmpc_command *c, void *stream)
{
    using namespace frp::command;
    if (!c || c->B < 1 || c->N < 2 || c->N > 64 || c->S < 1 || (long long)c->B * c->S > 0x7fffffffLL) return FRP_ERR_ARG;
    if (!positive(c->Ts) || !positive(c->mass) || !finite_d(c->g)) return FRP_ERR_ARG;
    if (!c->pre_plan || !c->t_cur || !c->status || !c->have_traj || !c->pub_end || !c->end_pt) return FRP_ERR_ARG;
    if (!c->cmd || !c->kind || !c->finish || !c->reset_output) return FRP_ERR_ARG;
    const int yaw_inputs = (c->odom != nullptr) + (c->init_yaw != nullptr) + (c->t_yaw != nullptr);
    if (yaw_inputs != 0 && yaw_inputs != 3) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    const int per_block = c->S >= THREADS ? 1 : THREADS / c->S; // whole planners per workgroup
    const unsigned blocks = (unsigned)(((long long)c->B + per_block - 1) / per_block);
    return launch(command_kernel, blocks, stream, *c, per_block);
}

} // extern "C"
