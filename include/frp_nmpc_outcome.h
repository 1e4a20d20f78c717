/* frp_nmpc.h section (10), frp_nmpc_outcome.h: the outcome of a tick on the device -- which planners run, whether a solve is accepted,
 * and the value NMPCSolver::solveNMPC returns.  frp_nmpc.h includes it, and including it alone works too (it pulls in frp_nmpc.h for
 * the error codes, FRP_MODEL_* and FRP_CMD_*, and carries its own extern "C").  Same ABI version: no existing struct changed, and a
 * library without these two symbols is refused by the loaders that need them (solver.OUTCOME_EXPORTS).
 *
 * What is restated (plan_manage/src/nmpc_solver.cpp unless another file is named):
 *     if (!exec_mpc_) return                                    nmpc_manage.cpp:52                 frp_nmpc_tick_begin (gate)
 *     cmd_status_ == WAIT -> 0, pub_end_ -> -1                  :355-356                           frp_nmpc_tick_begin (gate)
 *     !initialized_output_ || exit_code != 1 -> initMPCOutput   :363-364, :283                     frp_nmpc_tick_begin (keep)
 *     initialized_output_ = false                               :981 (the command timer)           frp_nmpc_tick_begin (reset_output)
 *     exit_code, fail_count_, replan_count_, update_result      :387-421                           frp_nmpc_tick_end   (accept)
 *     kino_replan_ raised by getCurTraj                         :136-140                           frp_nmpc_tick_end   (ref_replan)
 *     ref_end, max_index, the local end, switch_to_final        :435-447                           frp_nmpc_tick_end
 *     the return module                                         :452-481                           frp_nmpc_tick_end   (result)
 *     exec_mpc_ = false for 0, -2, -3                           nmpc_manage.cpp:60-97              frp_nmpc_tick_end   (exec_mpc)
 * What is NOT here: execFSMCallback, the transitions of checkReplanCallback, extforceCallback and plan_fail_count_ (nmpc_manage.cpp);
 * (those four are section (11), frp_nmpc_fsm.h, which shares exec_mpc, cmd_status and pub_end with this struct);
 * initMPCOutput's pre_mpc_output_ = mpc_output_ (:284) -- a cold start does not overwrite the command timer's snapshot; the clocks --
 * time_offset is the caller's.  The reference holds no test vectors for this rule: tests/outcome_oracle.py is a line-by-line
 * restatement, and the executable statement of what these two calls do.
 *
 * Both calls: every pointer is DEVICE memory, asynchronous on `stream`, nothing allocated, nothing read back, capturable into a
 * hipGraph with the tick; one launch each.  FRP_ERR_ARG before any device call, FRP_ERR_NO_DEVICE without a device. */
#ifndef FRP_NMPC_OUTCOME_H
#define FRP_NMPC_OUTCOME_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

/* gate[b]: why planner b does or does not solve this tick */
#define FRP_TICK_RUN 0    /* solveNMPC goes past :356                    */
#define FRP_TICK_IDLE 1   /* exec_mpc_ is false (nmpc_manage.cpp:52)     */
#define FRP_TICK_AT_END 2 /* cmd_status_ == WAIT: solveNMPC returns 0    */
#define FRP_TICK_ENDING 3 /* pub_end_: solveNMPC returns -1              */

/* result[b]: solveNMPC's return value (:345-349) -- 1 success, 0 at the global end, -1 reaching the global end, -2 replan, -3 odometry
 * far from the predicted state -- or, for a planner whose mpcCallback returned before calling it: */
#define FRP_TICK_RESULT_IDLE (-4)

typedef struct frp_nmpc_tick {
    int B;              /* planners                                                                                                 */
    /* state, in and out, int [B] each                                                                                              */
    int *fail_count;    /* fail_count_                                                                                              */
    int *replan_count;  /* replan_count_                                                                                            */
    int *kino_replan;   /* kino_replan_ (0 / 1)                                                                                     */
    int *exit_code;     /* the member exit_code: the exit flag of the last solve that RAN for this planner.  Not the solver's
                           exitflag array, which also holds the discarded solves of gated planners                                 */
    int *initialized;   /* initialized_output_                                                                                      */
    int *cmd_status;    /* cmd_status_, FRP_CMD_*: the array frp_nmpc_command.status walks                                          */
    int *pub_end;       /* pub_end_: frp_nmpc_command.pub_end                                                                       */
    double *cmd_end_pt; /* [B][3] cmd_end_pt_: frp_nmpc_command.end_pt                                                              */
    int *exec_mpc;      /* exec_mpc_, or NULL: every planner executes, and nothing is written                                       */
    /* scratch and outputs, int [B] each, every entry written by the call named                                                     */
    int *gate;          /* FRP_TICK_*                                                      frp_nmpc_tick_begin                       */
    int *keep;          /* 1: the plan stays, 0: cold start -- the `exitflag` argument of
                           frp_nmpc_coldstart_batch (a gated planner gets 1)               frp_nmpc_tick_begin                       */
    int *accept;        /* update_result (0 / 1): the `exitflag` argument of frp_nmpc_update_batch and the `accept` of
                           frp_nmpc_command_snapshot (a gated planner gets 0)              frp_nmpc_tick_end                         */
    int *result;        /* solveNMPC's return value, or FRP_TICK_RESULT_IDLE               frp_nmpc_tick_end                         */
    int *replan;        /* result == -2: the `active` mask of the next A*                  frp_nmpc_tick_end                         */
} frp_nmpc_tick;

/* mpcCallback's guard and the head of solveNMPC for B planners, BEFORE frp_nmpc_coldstart_batch:
 *   where reset_output != NULL and reset_output[b] != 0 (frp_nmpc_command.reset_output: PUB_END ran, :981): initialized <- 0 and
 *       reset_output[b] <- 0;
 *   gate <- IDLE where exec_mpc != NULL and exec_mpc[b] == 0, else AT_END where cmd_status == FRP_CMD_WAIT, else ENDING where pub_end
 *       != 0, else RUN;
 *   RUN: keep <- (initialized != 0 && exit_code == 1), then initialized <- 1 (:283).  Every other planner: keep <- 1 -- a planner that
 *       does not solve is never cold-started.
 * FRP_ERR_ARG: t NULL, B < 1, any array of t other than exec_mpc NULL (the outputs of frp_nmpc_tick_end included: one struct, checked
 * once the same way by both calls). */
int frp_nmpc_tick_begin(const frp_nmpc_tick *t, int *reset_output, void *stream);

typedef struct frp_nmpc_tick_in {
    int N, K;                  /* horizon (2 <= N <= 64), samples per kinodynamic path (>= 1)                                        */
    double Ts;                 /* nmpc_utils.h:189, finite and > 0                                                                  */
    const double *z;           /* [B][N][17] the solver's output of this tick                                                       */
    const int *exitflag;       /* [B] the solver's exit flags of this tick                                                          */
    const double *mpc_output;  /* [B][N+1][17] the plan BEFORE this tick's frp_nmpc_update_batch                                     */
    const double *state;       /* [B][9] stateMpc_: the odometry the tick started from                                              */
    const double *end_pt;      /* end_pt_, [3] or [B][3]                                                                            */
    int end_per_planner;
    const double *kino_path;   /* kino_path_, [K][3] or [B][K][3]                                                                   */
    int path_per_planner;
    const int *kino_size;      /* kino_size_, [1] or [B].  Compared as it is; as an index it is clamped to [1, K]                   */
    int size_per_planner;
    const double *time_offset; /* [B] (mpc_start_time_ - kino_start_time_).toSec() (:436): finite, and (N Ts + time_offset) / Ts
                                  within int -- the caller's contract, as the reference's (int) cast is undefined otherwise; such a
                                  value faults nothing here, and the max_index it yields is unspecified                             */
    const int *ref_replan;     /* [B] frp_nmpc_reference.replan of this tick                                                        */
    int *mode;                 /* [B] FRP_MODEL_* in and out, or NULL: switch_to_final is not kept                                   */
} frp_nmpc_tick_in;

/* The tail of solveNMPC and the state consequences of mpcCallback for B planners, AFTER the solve and BEFORE frp_nmpc_update_batch.
 * Gated planners (gate != RUN): result <- 0 (AT_END), -1 (ENDING), FRP_TICK_RESULT_IDLE (IDLE); accept <- 0, replan <- 0; an AT_END
 * planner's exec_mpc <- 0 (mpcCallback's case 0); nothing else is touched -- exit_code, the counters and mode stay.
 * RUN planners, in the reference's order:
 *   exit_code <- exitflag; kino_replan |= (ref_replan != 0)                                                            (:136-140, :387)
 *   exit_code == 1: fail_count <- 0, replan_count <- 0, accept.  Else fail_count += 1; then replan_count > 3 && exit_code == 0: both
 *       counters <- 0, accept; else fail_count > 2: fail_count <- 0, replan_count += 1, kino_replan <- 1               (:398-421)
 *   ref_end = the position (slots 8-10) of row N - 1 and row1 = that of row 1, of the plan as frp_nmpc_update_batch will leave it:
 *       of z where accepted, else of mpc_output (the yaw wrap does not touch positions)                                 (:435, :452)
 *   max_index = (int)((N * Ts + time_offset) / Ts), the expression of frp_nmpc_mode_batch                               (:436)
 *   max_index > 0.5 * kino_size && |end_pt - kino_path[kino_size - 1]| > 0.7: kino_replan <- 1                          (:439-443)
 *   mode != NULL and (max_index >= kino_size || |ref_end - end_pt| < 1.0): mode <- FRP_MODEL_FINAL (sticky) -- what
 *       frp_nmpc_mode_batch with radius 1.0 leaves when run after the update                                            (:446-447)
 *   |row1 - state[0:3]| > 2.0: cmd_status <- FRP_CMD_WAIT, result <- -3                                                 (:452-463)
 *   else |ref_end - end_pt| < 0.15: pub_end <- 1, cmd_end_pt <- end_pt, result <- -1                                    (:466-472)
 *   else kino_replan: kino_replan <- 0, result <- -2                                                                    (:475-479)
 *   else result <- 1.  A raised kino_replan survives a -3 or a -1, as in the reference.
 *   replan <- (result == -2); exec_mpc <- 0 for result -2 and -3 (nmpc_manage.cpp:78-93)
 * Norms are sqrt((d0 * d0 + d1 * d1) + d2 * d2), every operation rounded on its own.
 * FRP_ERR_ARG: t or in NULL, what frp_nmpc_tick_begin refuses, N outside [2, 64], K < 1, Ts not finite and positive, any array of
 * `in` other than mode NULL. */
int frp_nmpc_tick_end(const frp_nmpc_tick *t, const frp_nmpc_tick_in *in, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OUTCOME_H */
