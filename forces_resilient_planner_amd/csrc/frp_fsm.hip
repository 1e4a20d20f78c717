// frp_fsm.hip -- frp_nmpc.h section (11), frp_nmpc_fsm.h: NMPCManage (plan_manage/src/nmpc_manage.cpp, "NM") for B planners: the goal,
// force and safety callbacks, mpcCallback's switch, and execFSMCallback split around the kinodynamic A* (exec_begin_kernel with the
// head of NMPCSolver::getKinoPath, plan_manage/src/nmpc_solver.cpp:148-186; exec_end_kernel with its tail, :215-225).
//
//   * One thread per planner, 256 per workgroup, no LDS, no barrier: a planner's callbacks read and write its own entries alone.  Per
//     planner a dozen 4-byte flags and a few 24-byte vectors; exec_begin also reads two 136-byte plan rows where a planner replans from
//     its plan.  The kernels cost their launch.
//   * The replan start state is the command timer's sample of the same plan at the same time: frp_fleet.hpp's in_plan and plan_row for
//     position and velocity, its quaternion product and thrust column for the world acceleration.  No contraction in this file (the
//     build passes -ffp-contract=off as well).
//   * atan2, sin and cos are ocml's, within an ulp or two of libm's; the 0.8 yaw threshold is tested on the device's own atan2.
//   * Every index is bounded by what the entry points checked; the plan row index by the in_plan test made on the doubles.
//   * no atomics, no waiting between workgroups, no inline assembly; every store is a plain C++ store from a vector lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_fleet.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace fsm {

using namespace fleet;

// std::max(a, b) = (a < b) ? b : a
__device__ inline double smax(double a, double b) { return (a < b) ? b : a; }
// max(max(abs(x), abs(y)), abs(z)) (NM:371, :383)
__device__ inline double max_abs3(double x, double y, double z) { return smax(smax(fabs(x), fabs(y)), fabs(z)); }

// NM:481-493
__global__ __launch_bounds__(THREADS) void goal_kernel(frp_nmpc_fsm f, const double *goal, const int *fresh)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= f.B) return;
    if (fresh[b] == 0) return;
    const double *gp = goal + 3 * (size_t)b;
    if (gp[2] < -0.1) return; // NM:484
    f.trigger[b] = 1;         // NM:486
    f.have_target[b] = 1;     // NM:487
    double *e = f.end_pt + 3 * (size_t)b;
    e[0] = gp[0]; e[1] = gp[1]; e[2] = 1.2; // NM:489
}

// NM:366-418
__global__ __launch_bounds__(THREADS) void force_kernel(frp_nmpc_fsm f, const double *force, const int *fresh, double bound)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= f.B) return;
    if (fresh[b] == 0 || f.consider_force[b] == 0) return; // NM:369
    const double fx = force[3 * (size_t)b], fy = force[3 * (size_t)b + 1], fz = force[3 * (size_t)b + 2];
    double *ext = f.external_acc + 3 * (size_t)b, *last = f.last_external_acc + 3 * (size_t)b;
    const double diverse = max_abs3(fx, fy, fz); // NM:371
    if (diverse <= bound) {                      // NM:372-377
        ext[0] = 0.0; ext[1] = 0.0; ext[2] = 0.0;
        last[0] = fx; last[1] = fy; last[2] = fz;
        f.surpass_count[b] = 0;
        return;
    }
    ext[0] = fx; ext[1] = fy; ext[2] = fz; // NM:380
    const double surpass = max_abs3(last[0] - fx, last[1] - fy, last[2] - fz); // NM:382-383
    if (surpass > bound) { // NM:385
        const int count = f.surpass_count[b] + 1; // NM:391
        f.surpass_count[b] = count;
        if (count >= 1) { // NM:393
            f.replan_force_surpass[b] = 1;           // NM:396
            last[0] = fx; last[1] = fy; last[2] = fz; // NM:397
            if (f.have_target[b] != 0) f.state[b] = FRP_FSM_REPLAN_TRAJ; // NM:399-402
            if (surpass > 10.0) { // NM:404-409
                f.have_target[b] = 0;
                f.state[b] = FRP_FSM_WAIT_TARGET;
            }
        }
    } else {
        f.surpass_count[b] = 0; // NM:414
    }
}

// NM:60-97
__global__ __launch_bounds__(THREADS) void mpc_kernel(frp_nmpc_fsm f, const int *result)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= f.B) return;
    const int r = result[b];
    if (r == 0) { // NM:67-75
        f.exec_mpc[b] = 0;
        f.have_target[b] = 0;
        f.state[b] = FRP_FSM_WAIT_TARGET;
    } else if (r == -2) { // NM:82-88
        f.exec_mpc[b] = 0;
        f.state[b] = FRP_FSM_REPLAN_TRAJ;
    } else if (r == -3) { // NM:89-95
        f.exec_mpc[b] = 0;
        f.state[b] = FRP_FSM_WAIT_TARGET;
    }
}

// NM:318-325, :333-338
__global__ __launch_bounds__(THREADS) void safety_kernel(frp_nmpc_fsm f, const int *goal_blocked, const int *first_hit)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= f.B) return;
    int st = f.state[b];
    if (f.have_target[b] != 0 && goal_blocked[b] != 0) { // NM:289-291
        if (st == FRP_FSM_EXEC_TRAJ) {                   // NM:318-320
            st = FRP_FSM_REPLAN_TRAJ;
        } else { // NM:321-325
            f.have_target[b] = 0;
            st = FRP_FSM_WAIT_TARGET;
        }
    }
    if (f.have_traj[b] != 0 && first_hit[b] >= 0) st = FRP_FSM_REPLAN_TRAJ; // NM:329-338
    f.state[b] = st;
}

// eulerToRot(euler) * (0, 0, thrust) (nmpc_solver.cpp:554-564, :176-178): Matrix3d(qz * qy * qx) times the body thrust
__device__ inline void thrust_world(double roll, double pitch, double yaw, double thrust, double *out)
{
    const double hr = 0.5 * roll, hp = 0.5 * pitch, hy = 0.5 * yaw;
    const Quat qx = {cos(hr), sin(hr), 0.0, 0.0}, qy = {cos(hp), 0.0, sin(hp), 0.0}, qz = {cos(hy), 0.0, 0.0, sin(hy)};
    thrust_column(qmul(qmul(qz, qy), qx), thrust, out);
}

// NM:127-259 up to getKinoPath, nmpc_solver.cpp:148-186 and callInitYaw's stores (:232-235, :261)
__global__ __launch_bounds__(THREADS) void exec_begin_kernel(frp_nmpc_fsm f, frp_nmpc_fsm_exec_in in)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= f.B) return;
    const int st = f.state[b];
    const double *od = in.state + 9 * (size_t)b;
    int search = 0;
    if (st == FRP_FSM_INIT) { // NM:129-140
        if (f.have_odom[b] != 0 && f.have_target[b] != 0) f.state[b] = FRP_FSM_WAIT_TARGET;
    } else if (st == FRP_FSM_WAIT_TARGET) { // NM:142-155
        if (f.have_target[b] == 0) {
            f.consider_force[b] = 0;
        } else {
            f.state[b] = FRP_FSM_INIT_YAW;
            f.call_init_yaw[b] = 1;
        }
    } else if (st == FRP_FSM_INIT_YAW) { // NM:157-180
        if (f.call_init_yaw[b] != 0) {
            const double *e = f.end_pt + 3 * (size_t)b;
            const double d0 = e[0] - od[0], d1 = e[1] - od[1]; // NM:161
            const double yaw = atan2(d1, d0);                   // NM:162
            f.init_yaw[b] = yaw;
            if (fabs(od[8] - yaw) >= 0.8) { // NM:164-167 -> callInitYaw
                double *yo = f.yaw_odom + 9 * (size_t)b;
#pragma unroll
                for (int j = 0; j < 9; j++) yo[j] = od[j];   // :232
                f.pub_end[b] = 0;                            // :234
                f.change_yaw_time[b] = in.now[0];            // :235
                f.cmd_status[b] = FRP_CMD_ROTATE_YAW;        // :261
            }
            f.call_init_yaw[b] = 0; // NM:168-169
        } else if (fabs(od[8] - f.init_yaw[b]) < 0.8) { // NM:172-177
            f.consider_force[b] = 1;
            f.state[b] = FRP_FSM_GEN_NEW_TRAJ;
        }
    } else if (st == FRP_FSM_GEN_NEW_TRAJ || st == FRP_FSM_REPLAN_TRAJ) { // NM:182-245
        f.exec_mpc[b] = 0; // NM:184, :218
        if (f.plan_fail_count[b] > 3) { // NM:187-192, :220-225
            f.have_target[b] = 0;
            f.state[b] = FRP_FSM_WAIT_TARGET;
            f.plan_fail_count[b] = 0;
        } else {
            search = 1; // NM:194, :227
            double sp[3] = {od[0], od[1], od[2]}, sv[3] = {od[3], od[4], od[5]}, sa[3] = {0.0, 0.0, 0.0}; // :151-153
            const double t = in.t_cur[b];
            if (st == FRP_FSM_REPLAN_TRAJ && in.exit_code[b] == 1 && in_plan(t, in.Ts, in.N)) { // :160, :167
                double q[ROW]; // :164, :169-171, 0 <= t / Ts < N - 1
                plan_row(in.pre_plan, (size_t)b * in.N, plan_stage(t, in.Ts), plan_fraction(t, in.Ts), q);
                sp[0] = q[8]; sp[1] = q[9]; sp[2] = q[10];   // :173
                sv[0] = q[11]; sv[1] = q[12]; sv[2] = q[13]; // :174
                double tw[3];
                thrust_world(q[14], q[15], q[16], q[3], tw); // :176-178
                sa[0] = tw[0] / in.mass; sa[1] = tw[1] / in.mass; sa[2] = tw[2] / in.mass - in.g; // :178-180
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                in.start_pt[3 * (size_t)b + j] = sp[j];
                in.start_vel[3 * (size_t)b + j] = sv[j];
                in.start_acc[3 * (size_t)b + j] = sa[j];
                in.retry_pt[3 * (size_t)b + j] = od[j];      // :199
                in.retry_vel[3 * (size_t)b + j] = od[3 + j];
            }
        }
    } else if (st == FRP_FSM_EXEC_TRAJ) { // NM:247-257
        if (f.trigger[b] != 0 && f.exec_mpc[b] != 0) f.state[b] = FRP_FSM_REPLAN_TRAJ;
    }
    in.search[b] = search;
}

// NM:194-210, :227-242 and nmpc_solver.cpp:215-225
__global__ __launch_bounds__(THREADS) void exec_end_kernel(frp_nmpc_fsm f, const int *search, const int *astar_status, const double *now)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= f.B) return;
    if (search[b] == 0) return;
    if (astar_status[b] != FRP_ASTAR_NO_PATH) {
        if (f.mode) f.mode[b] = FRP_MODEL_NORMAL;  // :218
        f.kino_start_time[b] = now[0];             // :219
        f.cmd_status[b] = FRP_CMD_PUB_TRAJ;        // :222
        f.pub_end[b] = 0;                          // :223
        f.have_traj[b] = 1;                        // NM:197, :229
        f.trigger[b] = 0;                          // NM:198, :230
        f.exec_mpc[b] = 1;                         // NM:199, :231
        f.replan_force_surpass[b] = 0;             // NM:200, :232
        f.plan_fail_count[b] = 0;                  // NM:203, :235
        f.state[b] = FRP_FSM_EXEC_TRAJ;            // NM:204, :236
    } else {
        f.plan_fail_count[b] += 1;                 // NM:208, :240
        f.state[b] = FRP_FSM_GEN_NEW_TRAJ;         // NM:209, :241
    }
}

static bool fsm_ok(const frp_nmpc_fsm *f)
{
    return f && f->B >= 1 && f->state && f->have_odom && f->have_target && f->have_traj && f->trigger && f->call_init_yaw && f->consider_force &&
           f->replan_force_surpass && f->surpass_count && f->plan_fail_count && f->exec_mpc && f->cmd_status && f->pub_end && f->end_pt &&
           f->external_acc && f->last_external_acc && f->init_yaw && f->yaw_odom && f->change_yaw_time && f->kino_start_time;
}

} // namespace fsm
} // namespace frp

extern "C" {

int frp_nmpc_fsm_goal(const frp_nmpc_fsm *f, const double *goal, const int *fresh, void *stream)
{
    using namespace frp::fsm;
    if (!fsm_ok(f) || !goal || !fresh) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(goal_kernel, blocks_for(f->B), stream, *f, goal, fresh);
}

int frp_nmpc_fsm_force(const frp_nmpc_fsm *f, const double *force, const int *fresh, double ext_noise_bound, void *stream)
{
    using namespace frp::fsm;
    if (!fsm_ok(f) || !force || !fresh) return FRP_ERR_ARG;
    if (!non_negative(ext_noise_bound)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(force_kernel, blocks_for(f->B), stream, *f, force, fresh, ext_noise_bound);
}

int frp_nmpc_fsm_mpc(const frp_nmpc_fsm *f, const int *result, void *stream)
{
    using namespace frp::fsm;
    if (!fsm_ok(f) || !result) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(mpc_kernel, blocks_for(f->B), stream, *f, result);
}

int frp_nmpc_fsm_safety(const frp_nmpc_fsm *f, const int *goal_blocked, const int *first_hit, void *stream)
{
    using namespace frp::fsm;
    if (!fsm_ok(f) || !goal_blocked || !first_hit) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(safety_kernel, blocks_for(f->B), stream, *f, goal_blocked, first_hit);
}

int frp_nmpc_fsm_exec_begin(const frp_nmpc_fsm *f, const frp_nmpc_fsm_exec_in *in, void *stream)
{
    using namespace frp::fsm;
    if (!fsm_ok(f) || !in) return FRP_ERR_ARG;
    if (in->N < 2 || in->N > 64 || !positive(in->Ts) || !positive(in->mass) || !finite_d(in->g)) return FRP_ERR_ARG;
    if (!in->state || !in->pre_plan || !in->exit_code || !in->t_cur || !in->now) return FRP_ERR_ARG;
    if (!in->search || !in->start_pt || !in->start_vel || !in->start_acc || !in->retry_pt || !in->retry_vel) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(exec_begin_kernel, blocks_for(f->B), stream, *f, *in);
}

int frp_nmpc_fsm_exec_end(const frp_nmpc_fsm *f, const int *search, const int *astar_status, const double *now, void *stream)
{
    using namespace frp::fsm;
    if (!fsm_ok(f) || !search || !astar_status || !now) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(exec_end_kernel, blocks_for(f->B), stream, *f, search, astar_status, now);
}

} // extern "C"
