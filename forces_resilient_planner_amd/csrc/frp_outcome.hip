// frp_outcome.hip -- frp_nmpc.h section (10), frp_nmpc_outcome.h: the decision in the middle of NMPCSolver::solveNMPC
// (plan_manage/src/nmpc_solver.cpp:351-482) and of NMPCManage::mpcCallback (plan_manage/src/nmpc_manage.cpp:50-97) for B planners:
// who runs (tick_begin_kernel), whether the solve is accepted and what solveNMPC returns (tick_end_kernel).
//
//   * One thread per planner, 256 per workgroup, no LDS, no barrier: a planner's decision reads its own entries alone.  Per planner
//     about twenty 4-byte entries in and out, and six 24-byte positions (row 1 and row N - 1 of z or of the plan, the odometry, the
//     goal, the path's end); the kernels cost their launch.
//   * The three norms decide by comparison with a constant, so they are the reference's operations, one rounding each: no contraction
//     in this file (the build passes -ffp-contract=off as well), an IEEE sqrt.  max_index is frp_reference.hip's mode_kernel's
//     expression, converted by the same instruction.
//   * Every index is bounded by what the entry points checked; kino_size, which is device data, is clamped to [1, K] before it indexes
//     the path.
//   * no atomics, no waiting between workgroups, no inline assembly; every store is a plain C++ store from a vector lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_fleet.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace outcome {

using namespace fleet;

// Eigen's (a - b).norm() for three doubles: sqrt((d0 * d0 + d1 * d1) + d2 * d2)
__device__ inline double dist(const double *a, const double *b)
{
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

// nmpc_manage.cpp:52, nmpc_solver.cpp:355-356, :363-364 with :283, and the command timer's :981
__global__ __launch_bounds__(THREADS) void tick_begin_kernel(frp_nmpc_tick t, int *reset_output)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= t.B) return;
    int init = t.initialized[b];
    if (reset_output && reset_output[b] != 0) { // :981
        init = 0;
        reset_output[b] = 0;
    }
    int gate = FRP_TICK_RUN;
    if (t.exec_mpc && t.exec_mpc[b] == 0) gate = FRP_TICK_IDLE;   // nmpc_manage.cpp:52
    else if (t.cmd_status[b] == FRP_CMD_WAIT) gate = FRP_TICK_AT_END; // :355
    else if (t.pub_end[b] != 0) gate = FRP_TICK_ENDING;           // :356
    int keep = 1;
    if (gate == FRP_TICK_RUN) {
        keep = (init != 0 && t.exit_code[b] == 1); // :363
        init = 1;                                  // :283, or already true
    }
    t.gate[b] = gate;
    t.keep[b] = keep;
    t.initialized[b] = init;
}

// nmpc_solver.cpp:387-481 and nmpc_manage.cpp:60-97
__global__ __launch_bounds__(THREADS) void tick_end_kernel(frp_nmpc_tick t, frp_nmpc_tick_in in)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= t.B) return;
    const int gate = t.gate[b];
    if (gate != FRP_TICK_RUN) {
        t.result[b] = gate == FRP_TICK_AT_END ? 0 : gate == FRP_TICK_ENDING ? -1 : FRP_TICK_RESULT_IDLE;
        t.accept[b] = 0;
        t.replan[b] = 0;
        if (gate == FRP_TICK_AT_END && t.exec_mpc) t.exec_mpc[b] = 0; // nmpc_manage.cpp:66-73
        return;
    }
    const int N = in.N;
    const int exit_code = in.exitflag[b]; // :387, :394
    int fail = t.fail_count[b], rep = t.replan_count[b];
    int kino_replan = (t.kino_replan[b] != 0) | (in.ref_replan[b] != 0); // getCurTraj, :136-140
    int accept = 0;
    if (exit_code == 1) { // :398-404
        fail = 0; rep = 0; accept = 1;
    } else {
        fail += 1; // :407
        if (rep > 3 && exit_code == 0) { // :408-413
            fail = 0; rep = 0; accept = 1;
        } else if (fail > 2) { // :414-420
            fail = 0; rep += 1; kino_replan = 1;
        }
    }
    // the plan as the update will leave it (:423-429): its rows 1 and N - 1, positions only
    const double *rows = accept ? in.z + (size_t)b * N * ROW : in.mpc_output + (size_t)b * (N + 1) * ROW;
    const double *ref_end = rows + (size_t)(N - 1) * ROW + 8, *row1 = rows + ROW + 8; // :435, :452
    const double *end_pt = in.end_pt + (in.end_per_planner ? 3 * (size_t)b : 0);
    const int kino_size = in.kino_size[in.size_per_planner ? b : 0];
    const int max_index = (int)((N * in.Ts + in.time_offset[b]) / in.Ts); // :436
    const int last = kino_size < 1 ? 0 : (kino_size > in.K ? in.K : kino_size) - 1;
    const double *path_end = in.kino_path + ((in.path_per_planner ? (size_t)b * in.K : 0) + last) * 3;
    if (max_index > 0.5 * kino_size && dist(end_pt, path_end) > 0.7) kino_replan = 1; // :439-443
    const double to_goal = dist(ref_end, end_pt);
    if (in.mode && (max_index >= kino_size || to_goal < 1.0)) in.mode[b] = FRP_MODEL_FINAL; // :446-447
    int result = 1;
    if (dist(row1, in.state + 9 * (size_t)b) > 2.0) { // :452-463
        t.cmd_status[b] = FRP_CMD_WAIT;
        result = -3;
    } else if (to_goal < 0.15) { // :466-472
        t.pub_end[b] = 1;
        t.cmd_end_pt[3 * (size_t)b] = end_pt[0]; t.cmd_end_pt[3 * (size_t)b + 1] = end_pt[1]; t.cmd_end_pt[3 * (size_t)b + 2] = end_pt[2];
        result = -1;
    } else if (kino_replan) { // :475-479
        kino_replan = 0;
        result = -2;
    }
    t.exit_code[b] = exit_code;
    t.fail_count[b] = fail;
    t.replan_count[b] = rep;
    t.kino_replan[b] = kino_replan;
    t.accept[b] = accept;
    t.result[b] = result;
    t.replan[b] = result == -2;
    if (t.exec_mpc && (result == -2 || result == -3)) t.exec_mpc[b] = 0; // nmpc_manage.cpp:78-93
}

static bool tick_ok(const frp_nmpc_tick *t)
{
    return t && t->B >= 1 && t->fail_count && t->replan_count && t->kino_replan && t->exit_code && t->initialized && t->cmd_status && t->pub_end &&
           t->cmd_end_pt && t->gate && t->keep && t->accept && t->result && t->replan;
}

} // namespace outcome
} // namespace frp

extern "C" {

int frp_nmpc_tick_begin(const frp_nmpc_tick *t, int *reset_output, void *stream)
{
    using namespace frp::outcome;
    if (!tick_ok(t)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(tick_begin_kernel, blocks_for(t->B), stream, *t, reset_output);
}

int frp_nmpc_tick_end(const frp_nmpc_tick *t, const frp_nmpc_tick_in *in, void *stream)
{
    using namespace frp::outcome;
    if (!tick_ok(t) || !in) return FRP_ERR_ARG;
    if (in->N < 2 || in->N > 64 || in->K < 1 || !positive(in->Ts)) return FRP_ERR_ARG;
    if (!in->z || !in->exitflag || !in->mpc_output || !in->state || !in->end_pt || !in->kino_path || !in->kino_size || !in->time_offset || !in->ref_replan)
        return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(tick_end_kernel, blocks_for(t->B), stream, *t, *in);
}

} // extern "C"
