/* frp_nmpc.h section (11), frp_nmpc_fsm.h: the fleet's state machine on the device -- NMPCManage (plan_manage/src/nmpc_manage.cpp, "NM"
 * below): goals, external forces, the safety timer's transitions, the consequences of solveNMPC's return value, and execFSMCallback
 * with the head and tail of NMPCSolver::getKinoPath around the kinodynamic A*.  frp_nmpc.h includes it, and including it alone works
 * too (it pulls in frp_nmpc.h for the error codes, FRP_MODEL_*, FRP_CMD_*, FRP_ASTAR_* and FRP_TICK_RESULT_IDLE, and carries its own
 * extern "C").  Same ABI version: no existing struct changed, and a library without these six symbols is refused by the loaders that
 * need them (solver.FSM_EXPORTS).
 *
 * What is restated:
 *     goalCallback                                              NM:481-493                         frp_nmpc_fsm_goal
 *     extforceCallback                                          NM:366-418                         frp_nmpc_fsm_force
 *     mpcCallback's switch on solveNMPC's return value          NM:60-97                           frp_nmpc_fsm_mpc
 *     checkReplanCallback's transitions                         NM:318-325, :333-338               frp_nmpc_fsm_safety
 *     execFSMCallback up to the call of getKinoPath             NM:127-259                         frp_nmpc_fsm_exec_begin
 *     callInitYaw's stores                                      nmpc_solver.cpp:232-235, :261      frp_nmpc_fsm_exec_begin
 *     getKinoPath's start state                                 nmpc_solver.cpp:148-186            frp_nmpc_fsm_exec_begin
 *     what execFSMCallback does with getKinoPath's verdict      NM:194-210, :227-242               frp_nmpc_fsm_exec_end
 *     getKinoPath's tail                                        nmpc_solver.cpp:215-225            frp_nmpc_fsm_exec_end
 * What is NOT restated:
 *     the clocks: `now` and `t_cur` are the caller's;
 *     the odometry callbacks (NM:421-478): have_odom and `state` are the caller's;
 *     prints, displayPath, displayGoalPoint, and the two sleeps of mpcCallback (NM:72, :79);
 *     the reference's unsynchronised four-thread spinner: on the device a planner's callbacks happen in the order of the calls;
 *     the collision checks and the goal search themselves (frp_nmpc_occmap_check.h), the A* (frp_nmpc_astar_batch), init_yaw_dot_
 *     (frp_nmpc_command_batch derives it from yaw_odom and init_yaw).
 * The reference leaves end_pt_, external_acc_, last_external_acc_ and init_yaw_ uninitialised; a caller of this header starts them at 0
 * (solver.FleetFSM does).  NMPCManage::init_yaw_ and NMPCSolver::init_yaw_ are one array here: the solver's copy is read by the command
 * timer in ROTATE_YAW alone, a state only callInitYaw enters, and callInitYaw stores the manager's value.
 * This layer is STRUCTURALLY UNPINNED: the reference holds no test vectors for it.  tests/fsm_oracle.py is a line-by-line restatement,
 * pinned by the hand-worked scenarios of tests/test_fsm_cpu.py, and the executable statement of what these calls do.
 *
 * Every call: every pointer is DEVICE memory, asynchronous on `stream`, nothing allocated, nothing read back, capturable into a
 * hipGraph with the tick; one launch, one thread per planner.  FRP_ERR_ARG before any device call, FRP_ERR_NO_DEVICE without a device. */
#ifndef FRP_NMPC_FSM_H
#define FRP_NMPC_FSM_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

/* enum FSM_EXEC_STATE (plan_manage/nmpc_manage.h), in its order */
#define FRP_FSM_INIT 0
#define FRP_FSM_WAIT_TARGET 1
#define FRP_FSM_INIT_YAW 2
#define FRP_FSM_GEN_NEW_TRAJ 3
#define FRP_FSM_REPLAN_TRAJ 4
#define FRP_FSM_EXEC_TRAJ 5

typedef struct frp_nmpc_fsm {
    int B;                     /* planners                                                                                          */
    /* NMPCManage's members, int [B] each, in and out; as the constructor and init leave them: state INIT, everything else 0        */
    int *state;                /* exec_state_, FRP_FSM_*                                                                            */
    int *have_odom;            /* have_odom_: written by the caller alone (the odometry callbacks are not restated)                 */
    int *have_target;          /* have_target_: the have_target of frp_nmpc_occmap_check_goals                                      */
    int *have_traj;            /* have_traj_ (NMPCManage's: a kinodynamic path exists): the have_traj of frp_nmpc_occmap_check_paths.
                                  NOT have_mpc_traj_, which is frp_nmpc_command.have_traj                                           */
    int *trigger;              /* trigger_                                                                                          */
    int *call_init_yaw;        /* call_init_yaw_                                                                                    */
    int *consider_force;       /* consider_force_                                                                                   */
    int *replan_force_surpass; /* replan_force_surpass_                                                                             */
    int *surpass_count;        /* surpass_count_                                                                                    */
    int *plan_fail_count;      /* plan_fail_count_                                                                                  */
    int *exec_mpc;             /* exec_mpc_: the array frp_nmpc_tick.exec_mpc.  Starts at 0 under this state machine (NM's
                                  exec_mpc_ = false); the first successful search raises it                                        */
    /* the NMPCSolver members the state machine writes through callInitYaw and getKinoPath                                          */
    int *cmd_status;           /* cmd_status_: frp_nmpc_tick.cmd_status = frp_nmpc_command.status                                   */
    int *pub_end;              /* pub_end_: frp_nmpc_tick.pub_end = frp_nmpc_command.pub_end                                        */
    /* double                                                                                                                       */
    double *end_pt;            /* [B][3] end_pt_: the goal -- the end_pt of the safety checks (which may move it), of the A*, of
                                  frp_nmpc_tick_in                                                                                  */
    double *external_acc;      /* [B][3] external_acc_: the external_acc of the A* and of the pack                                  */
    double *last_external_acc; /* [B][3] last_external_acc_                                                                         */
    double *init_yaw;          /* [B] init_yaw_: frp_nmpc_command.init_yaw                                                          */
    double *yaw_odom;          /* [B][9] realOdom_ as callInitYaw stored it: frp_nmpc_command.odom                                  */
    double *change_yaw_time;   /* [B] change_yaw_time_, on the caller's clock: t_yaw = now - change_yaw_time                        */
    double *kino_start_time;   /* [B] kino_start_time_, on the caller's clock: time_offset = mpc_start_time - kino_start_time       */
    int *mode;                 /* [B] FRP_MODEL_*, or NULL: switch_to_final = false (nmpc_solver.cpp:218) is not kept               */
} frp_nmpc_fsm;

/* goalCallback (NM:481-493) for B planners: goal [B][3], fresh [B] (non-zero: a message arrived for this planner).  Where fresh and
 * NOT goal.z < -0.1 (a NaN z is no such z: the goal is taken, as written): trigger <- 1, have_target <- 1, end_pt <- (goal.x, goal.y,
 * 1.2).  FRP_ERR_ARG: f NULL, B < 1, any array of f other than mode NULL (one struct, checked the same way by all six calls), goal or
 * fresh NULL. */
int frp_nmpc_fsm_goal(const frp_nmpc_fsm *f, const double *goal, const int *fresh, void *stream);

/* extforceCallback (NM:366-418) for B planners: force [B][3] (mass-normalised), fresh [B].  Only where fresh and consider_force:
 *   diverse = max(max(|fx|, |fy|), |fz|) with std::max's (a < b) ? b : a, in that nesting (NM:371)
 *   diverse <= ext_noise_bound (quiet): external_acc <- 0, last_external_acc <- force, surpass_count <- 0          (NM:374-376)
 *   else (loud, a NaN force included): external_acc <- force; diff = last_external_acc - external_acc; surpass = the same max of
 *       |diff|; surpass > ext_noise_bound: surpass_count += 1 and, where surpass_count >= 1: replan_force_surpass <- 1,
 *       last_external_acc <- force, state <- REPLAN_TRAJ where have_target, THEN surpass > 10.0: have_target <- 0, state <-
 *       WAIT_TARGET -- in that order, so the second wins; else surpass_count <- 0                                  (NM:380-415)
 * FRP_ERR_ARG: what frp_nmpc_fsm_goal refuses; ext_noise_bound (nmpc/ext_noise_bound, 0.5) not finite or negative. */
int frp_nmpc_fsm_force(const frp_nmpc_fsm *f, const double *force, const int *fresh, double ext_noise_bound, void *stream);

/* The switch of mpcCallback (NM:60-97) on result [B] = frp_nmpc_tick.result:  0: exec_mpc <- 0, have_target <- 0, state <-
 * WAIT_TARGET;  -2: exec_mpc <- 0, state <- REPLAN_TRAJ;  -3: exec_mpc <- 0, state <- WAIT_TARGET;  1, -1, FRP_TICK_RESULT_IDLE and
 * any other value: nothing.  (frp_nmpc_tick_end has cleared exec_mpc for 0, -2 and -3 already; the stores here are the same.) */
int frp_nmpc_fsm_mpc(const frp_nmpc_fsm *f, const int *result, void *stream);

/* The transitions of checkReplanCallback (NM:318-325, :333-338).  goal_blocked [B] and first_hit [B] are the outputs of
 * frp_nmpc_occmap_check_goals / frp_nmpc_occmap_check_paths run on f.end_pt, f.have_target and f.have_traj:
 *   have_target && goal_blocked: EXEC_TRAJ -> REPLAN_TRAJ; any other state: have_target <- 0, state <- WAIT_TARGET -- whether or not
 *       the search moved the goal (its have_target_ = true, NM:310, is overwritten by NM:322);
 *   then have_traj && first_hit >= 0: state <- REPLAN_TRAJ from ANY state, as written (a WAIT_TARGET planner included). */
int frp_nmpc_fsm_safety(const frp_nmpc_fsm *f, const int *goal_blocked, const int *first_hit, void *stream);

typedef struct frp_nmpc_fsm_exec_in {
    int N;                     /* horizon (2 <= N <= 64)                                                                            */
    double Ts, mass, g;        /* nmpc_utils.h:189, nmpc/mass, the g of nmpc_solver.cpp: Ts and mass finite and > 0, g finite       */
    const double *state;       /* [B][9] stateOdom_: position 0-2, velocity 3-5, euler 6-8                                          */
    const double *pre_plan;    /* [B][N][17] pre_mpc_output_ (frp_nmpc_command_snapshot)                                            */
    const int *exit_code;      /* [B] frp_nmpc_tick.exit_code                                                                       */
    const double *t_cur;       /* [B] (now - pre_mpc_start_time_).toSec() (nmpc_solver.cpp:163)                                     */
    const double *now;         /* [1] ros::Time::now() of this step, on the caller's clock                                          */
    /* outputs: search, and -- for the planners that search alone -- the A*'s own start buffers                                     */
    int *search;               /* [B] 1: this planner calls getKinoPath in this step (the `active` of frp_nmpc_astar_batch), else 0  */
    double *start_pt, *start_vel, *start_acc; /* [B][3] each: frp_nmpc_astar.start_pt / start_vel / start_acc                       */
    double *retry_pt, *retry_vel;             /* [B][3] each: frp_nmpc_astar.retry_pt / retry_vel                                   */
} frp_nmpc_fsm_exec_in;

/* One execFSMCallback (NM:127-259) for B planners up to the call of getKinoPath, and that function's head:
 *   INIT          !have_odom: nothing; else have_target: state <- WAIT_TARGET
 *   WAIT_TARGET   !have_target: consider_force <- 0; else state <- INIT_YAW, call_init_yaw <- 1
 *   INIT_YAW      call_init_yaw: init_yaw <- atan2(end_pt.y - state[1], end_pt.x - state[0]); where |state[8] - init_yaw| >= 0.8,
 *                 callInitYaw: yaw_odom <- state, pub_end <- 0, change_yaw_time <- now, cmd_status <- FRP_CMD_ROTATE_YAW; then
 *                 call_init_yaw <- 0 and nothing else in this step.  Otherwise |state[8] - init_yaw| < 0.8: consider_force <- 1,
 *                 state <- GEN_NEW_TRAJ
 *   GEN_NEW_TRAJ, REPLAN_TRAJ   exec_mpc <- 0; plan_fail_count > 3: have_target <- 0, state <- WAIT_TARGET, plan_fail_count <- 0;
 *                 else search <- 1 and the start state is written
 *   EXEC_TRAJ     trigger && exec_mpc: state <- REPLAN_TRAJ
 * Every planner that does not search gets search <- 0 and its five A* rows are NOT written.
 * The start state (nmpc_solver.cpp:151-186): where the step is REPLAN_TRAJ, exit_code == 1, t_cur >= 0 and t_cur / Ts < N - 1 (the test
 * of frp_nmpc_command_batch, on the doubles: a NaN or a quotient beyond int takes the other branch), the row  pre_plan[i] + fmod(t_cur, Ts)
 * / Ts * (pre_plan[i + 1] - pre_plan[i]),  i = (int)(t_cur / Ts), one rounding per operation as in frp_nmpc_command_batch: start_pt =
 * slots 8-10, start_vel = slots 11-13 (both the host's bits), start_acc = eulerToRot(slots 14-16) * (0, 0, slot 3) / mass with g
 * subtracted from z.  Otherwise start_pt = state 0-2, start_vel = state 3-5, start_acc = 0.  retry_pt / retry_vel = state 0-2 / 3-5 always.
 * FRP_ERR_ARG: what frp_nmpc_fsm_goal refuses; in NULL, N outside [2, 64], Ts or mass not finite and positive, g not finite, any array
 * of `in` NULL. */
int frp_nmpc_fsm_exec_begin(const frp_nmpc_fsm *f, const frp_nmpc_fsm_exec_in *in, void *stream);

/* The rest of that execFSMCallback, after frp_nmpc_astar_batch ran with active = search: astar_status [B] = frp_nmpc_astar.status.
 *   search != 0 and astar_status != FRP_ASTAR_NO_PATH: have_traj <- 1, trigger <- 0, exec_mpc <- 1, replan_force_surpass <- 0,
 *       plan_fail_count <- 0, state <- EXEC_TRAJ (NM:196-204, :228-236); kino_start_time <- now, mode <- FRP_MODEL_NORMAL where mode is
 *       given, cmd_status <- FRP_CMD_PUB_TRAJ, pub_end <- 0 (nmpc_solver.cpp:218-223)
 *   search != 0 and NO_PATH: plan_fail_count += 1, state <- GEN_NEW_TRAJ -- from REPLAN_TRAJ too, as written (NM:208-209, :240-241)
 *   search == 0: nothing.
 * FRP_ERR_ARG: what frp_nmpc_fsm_goal refuses; search, astar_status or now NULL. */
int frp_nmpc_fsm_exec_end(const frp_nmpc_fsm *f, const int *search, const int *astar_status, const double *now, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_FSM_H */
