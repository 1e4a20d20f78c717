/* frp_nmpc.h section (9), frp_nmpc_command.h: the planner's 100 Hz command timer on the device.  frp_nmpc.h includes it, and including it
 * alone works too (it pulls in frp_nmpc.h for the error codes and carries its own extern "C").  Same ABI version: the version
 * number guards the layout of the structs a caller may already have compiled (frp_nmpc.h, FRP_NMPC_ABI_VERSION), no existing struct
 * changed, and a library without these two symbols is refused by the loaders that need them (solver.COMMAND_EXPORTS).
 *
 * What is restated: NMPCSolver::cmdTrajCallback (plan_manage/src/nmpc_solver.cpp:865-987), the timer that turns the last accepted
 * plan pre_mpc_output_ into what the vehicle is told, with the pieces it leans on:
 *     pre_mpc_output_ = mpc_output_; have_mpc_traj_ = true      updateFORCESResults, :527-528      frp_nmpc_command_snapshot
 *     init_yaw_dot_                                             callInitYaw, :237-257              frp_nmpc_command_batch
 *     eulerToRot                                                :554-564                           frp_nmpc_command_batch
 *     CMD_STATUS                                                plan_manage/nmpc_utils.h:115-122   FRP_CMD_*
 * What is NOT here: whether a solve is accepted (fail_count_ / replan_count_, :398-421) -- the caller hands over the mask, and
 * frp_nmpc_tick_end (frp_nmpc_outcome.h) computes the reference's on the device, together with pub_end_ and cmd_end_pt_; the FSM
 * that calls callInitYaw (section (11), frp_nmpc_fsm.h: frp_nmpc_fsm_exec_begin writes odom, init_yaw and the ROTATE_YAW status); the clock -- t_cur and t_yaw are the caller's; ROS messages.  mav_msgs is not part of
 * the reference tree, so msgMultiDofJointTrajectoryFromPositionYaw (:889) is not restated: a ROTATE_YAW sample carries the position,
 * the yaw and the quaternion of a rotation about z by it, and the caller fills its message from them.
 * tests/command_oracle.py is the executable statement.
 *
 * Both calls: every pointer is DEVICE memory, asynchronous on `stream`, nothing allocated, nothing read back, capturable into a
 * hipGraph with the tick.  FRP_ERR_ARG before any device call, FRP_ERR_NO_DEVICE without a device. */
#ifndef FRP_NMPC_COMMAND_H
#define FRP_NMPC_COMMAND_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

/* enum CMD_STATUS (nmpc_utils.h:115-122), in its order */
#define FRP_CMD_INIT_POSITION 0
#define FRP_CMD_ROTATE_YAW 1
#define FRP_CMD_PUB_END 2
#define FRP_CMD_PUB_TRAJ 3
#define FRP_CMD_WAIT 4

/* kind[b][s]: what callback s of planner b published */
#define FRP_COMMAND_NONE 0        /* nothing: cmd = 16 zeros                                                     */
#define FRP_COMMAND_TRAJ 1        /* a trajectory point (PUB_TRAJ, :909-947)                                     */
#define FRP_COMMAND_END 2         /* the end point (PUB_END, :956-985)                                           */
#define FRP_COMMAND_YAW 3         /* position + yaw (ROTATE_YAW, :883-893)                                       */
#define FRP_COMMAND_NO_YAW_INPUT (-1) /* ROTATE_YAW met without odom / init_yaw / t_yaw: see frp_nmpc_command.odom */

#define FRP_COMMAND_STRIDE 16 /* doubles per sample of cmd: position 0-2, quaternion x y z w 3-6, linear velocity 7-9, body rates 10-12,
                                 linear acceleration 13-15 */

/* pre_mpc_output_ = mpc_output_; have_mpc_traj_ = true (:527-528, reached through :423-428) for B planners: where accept[b] != 0,
 * pre_plan[b][0..N-1][17] <- z[b] (the solver's output as it is: the copy is made BEFORE :531-543 wrap the yaw and duplicate the last
 * row, so pre_plan is not frp_nmpc_update_batch's mpc_output) and have_traj[b] <- 1; every other planner keeps its snapshot and
 * its flag.  accept == NULL is FRP_ERR_ARG: which results are accepted is the caller's policy (exitflag == 1 is only the first
 * branch of :398-421).  FRP_ERR_ARG as well for B < 1, N outside [2, 64] or another NULL array. */
int frp_nmpc_command_snapshot(int B, int N, const double *z, const int *accept, double *pre_plan, int *have_traj, void *stream);

typedef struct frp_nmpc_command {
    int B, N, S;              /* planners, horizon (2 <= N <= 64), consecutive timer callbacks per planner (>= 1)                   */
    double Ts, mass, g;       /* nmpc_utils.h:189, nmpc/mass, the file's g (9.81); Ts and mass finite and > 0, g finite            */
    const double *pre_plan;   /* [B][N][17] pre_mpc_output_ (frp_nmpc_command_snapshot)                                             */
    const double *t_cur;      /* [B][S] (time_now - pre_mpc_start_time_).toSec() of every callback (:906)                           */
    int *status;              /* [B] in and out: cmd_status_, FRP_CMD_*; any other value publishes nothing and stays                 */
    const int *have_traj;     /* [B] have_mpc_traj_                                                                                 */
    const int *pub_end;       /* [B] pub_end_                                                                                       */
    const double *end_pt;     /* [B][3] cmd_end_pt_                                                                                 */
    /* The yaw rotation.  All three or none: a partial set is FRP_ERR_ARG.  With none the call never reads them, and a planner found
       in ROTATE_YAW -- the library cannot see that on the host -- gets the per-sample form of FRP_ERR_ARG: kind =
       FRP_COMMAND_NO_YAW_INPUT, 16 zeros, its status kept.                                                                         */
    const double *odom;       /* [B][9] realOdom_ as callInitYaw stored it: position 0-2, yaw 8 (:232)                              */
    const double *init_yaw;   /* [B] init_yaw_ (:233)                                                                               */
    const double *t_yaw;      /* [B][S] (now - change_yaw_time_).toSec() of every callback (:885)                                   */
    /* outputs                                                                                                                      */
    double *cmd;              /* [B][S][FRP_COMMAND_STRIDE]; a callback that publishes nothing writes 16 zeros                       */
    int *kind;                /* [B][S] FRP_COMMAND_*                                                                               */
    int *finish;              /* [B] finish_mpc_cmd_ after the last callback: 0 / 1 as the last PUB_TRAJ callback with a trajectory
                                 left it (:946, :950), NOT written when no callback touched it                                      */
    int *reset_output;        /* [B] <- 1 where PUB_END ran (initialized_output_ = false, :981: cold-start that planner), NOT written
                                 elsewhere                                                                                          */
} frp_nmpc_command;

/* S consecutive cmdTrajCallback calls for each of B planners in ONE launch; callback s + 1 sees the status callback s left.
 *   INIT_POSITION, WAIT (:878-881, :895-898)   nothing.
 *   PUB_TRAJ (:900-954)   have_traj[b] == 0: nothing.  Otherwise with t = t_cur[b][s]: when (int)(t / Ts) < N - 1 && t >= 0 the
 *       row  pre_plan[i] + fmod(t, Ts) / Ts * (pre_plan[i + 1] - pre_plan[i]),  i = (int)(t / Ts), is published (one rounding per
 *       operation, an IEEE division and an exact fmod: index, fraction and the interpolated slots are the host's to the bit):
 *       position = row 8-10, velocity = row 11-13, rates = row 0-2, acceleration = eulerToRot(row 14-16) * (0, 0, row 3) / mass with
 *       g subtracted from z (:925-931), quaternion = AngleAxis(roll, X) * AngleAxis(pitch, Y) * AngleAxis(yaw, Z) (:933 -- the
 *       OPPOSITE order to eulerToRot's qz * qy * qx, as written there); finish <- 0.  Else finish <- 1 and, where pub_end[b] != 0,
 *       status <- PUB_END.  The test is made on the doubles, t >= 0 && t / Ts < N - 1, before any conversion: the same verdict for
 *       every t the reference's cast is defined for, and a NaN or a t / Ts beyond int -- where the reference's (int) is undefined
 *       behaviour -- takes the else branch and is never used as an index.
 *   PUB_END (:956-985)   end_pt with zero velocity, rates and acceleration, the attitude of row N - 1 (the reference's .at(19)) in
 *       the same X * Y * Z order, whatever have_traj says; then status <- WAIT and reset_output <- 1.
 *   ROTATE_YAW (:883-893)   d = init_yaw - odom[8]; init_yaw_dot = d > PI ? 2 PI - d : d < -PI ? d + 2 PI : d with PI = 3.1415926
 *       (:3), clamped to +-0.4 PI (:239-257, the first fold as written: it yields 2 PI - d, not d - 2 PI); yaw_temp = odom[8] +
 *       t_yaw * init_yaw_dot; desired_yaw = d >= 0 ? std::min(yaw_temp, init_yaw) : std::max(yaw_temp, init_yaw), with std::min /
 *       std::max's (b < a) ? b : a and (a < b) ? b : a.  Published: position = odom 0-2, quaternion (0, 0, sin(yaw / 2),
 *       cos(yaw / 2)), desired_yaw itself in slot 12, everything else 0.  The status stays (the FSM leaves this state, not the timer).
 * FRP_ERR_ARG: c or any array other than the yaw inputs NULL, B < 1, N outside [2, 64], S < 1, B * S beyond 2^31 - 1, Ts or mass
 * not finite and positive, g not finite, a partial set of yaw inputs. */
int frp_nmpc_command_batch(const frp_nmpc_command *c, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_COMMAND_H */
