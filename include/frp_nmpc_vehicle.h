/* frp_nmpc.h section (12), frp_nmpc_vehicle.h: the vehicle on the device -- a tracking plant that flies the command timer's samples, and
 * the reference's two odometry callbacks that turn what it flew into the planner's `state`.  With it a simulated fleet closes its loop
 * in device memory: commands -> plant -> message -> callback -> state, period after period in one captured graph.  frp_nmpc.h includes
 * it, and including it alone works too (it pulls in frp_nmpc.h for the error codes and FRP_COMMAND_*, and carries its own extern "C").
 * Same ABI version: no existing struct changed, and a library without these four symbols is refused by the loaders that need them
 * (solver.VEHICLE_EXPORTS).
 *
 * What is restated from the reference:
 *     odometryCallback                                          plan_manage/src/nmpc_manage.cpp:421-448     frp_nmpc_vehicle_odometry, FRP_ODOM_WORLD
 *     odometryTransCallback                                     plan_manage/src/nmpc_manage.cpp:456-478     frp_nmpc_vehicle_odometry, FRP_ODOM_BODY
 *     the dynamics                                              matlab_code/dynamics/nonlinear_dynamics.m:21-40, as csrc/frp_model.hpp's accel()
 *                                                               holds them, pinned to the reference's CasADi callbacks   frp_nmpc_vehicle_step
 *     eulerToRot's quaternion qz * qy * qx                      plan_manage/src/nmpc_solver.cpp:554-564      frp_nmpc_vehicle_message
 * What has NO counterpart in the reference (it flies RotorS, which is not in its tree):
 *     the controller of frp_nmpc_vehicle_step, and the choice of the integrator and its step (Heun, the scheme transit.m:7-8 uses for
 *     the planner's own prediction, at dt_cmd / n_sub instead of 0.05 s);
 *     what the vehicle tracks while the timer publishes nothing (`hold`: a position hold);
 *     the message producer.
 * mav_msgs is not part of the reference tree either: getEulerAnglesFromQuaternion is restated from the formula of its public header and
 * eigenOdometryFromMsg as the copy it is, so the callbacks are STRUCTURALLY UNPINNED (no test vector of the reference reaches them).
 * odomT / tOdom (the message stamps, :425-426, :459-460) are read by nothing in the reference and are not kept.
 * tests/vehicle_oracle.py is the executable statement; tests/golden/vehicle_mp.npz the same scheme in 50 digits.
 *
 * Every call: every pointer is DEVICE memory, asynchronous on `stream`, nothing allocated, nothing read back, capturable into a
 * hipGraph with the tick; one launch, one thread per vehicle, 256 per workgroup, no kernel waits on another workgroup.  FRP_ERR_ARG
 * before any device call, FRP_ERR_NO_DEVICE without a device. */
#ifndef FRP_NMPC_VEHICLE_H
#define FRP_NMPC_VEHICLE_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

#define FRP_VEHICLE_STATE 9        /* doubles per vehicle of x: position 0-2, velocity 3-5 (world frame), roll pitch yaw 6-8 (ZYX): the model's state */
#define FRP_VEHICLE_HOLD_STRIDE 8  /* doubles per vehicle of hold: position 0-2, yaw 3, 4-7 written as 0 (one vehicle, one 64-byte line) */
#define FRP_VEHICLE_MSG_STRIDE 13  /* doubles per message: position 0-2, quaternion x y z w 3-6, linear twist 7-9, angular twist 10-12 */
#define FRP_VEHICLE_MAX_SUB 16     /* largest n_sub                                                                                     */

/* which callback a message is for: the frame of its linear twist */
#define FRP_ODOM_WORLD 1 /* odometryCallback: the twist is the world-frame velocity                                   */
#define FRP_ODOM_BODY 2  /* odometryTransCallback: the twist is in the body frame, the callback rotates it by R(q)   */

/* sat[b][s]: the clamps that engaged in sample s, and the two special branches */
#define FRP_VEHICLE_SAT_THRUST_LO 1
#define FRP_VEHICLE_SAT_THRUST_HI 2
#define FRP_VEHICLE_SAT_ROLL 4
#define FRP_VEHICLE_SAT_PITCH 8
#define FRP_VEHICLE_SAT_RATE0 16   /* RATE0 << i: body rate i                                     */
#define FRP_VEHICLE_SAT_ZERO_ACC 128 /* the commanded acceleration was exactly 0: zB = e3          */
#define FRP_VEHICLE_SAT_YAW_WRAP 256 /* the yaw error was moved into (-pi, pi]                     */

typedef struct frp_nmpc_vehicle {
    int B, S, n_sub;        /* vehicles, command samples per call (>= 1), Heun steps per sample (1 ... FRP_VEHICLE_MAX_SUB)           */
    double mass, g, dt_cmd; /* what the CONTROLLER is told (the plant's mass, drag and gravity are frp_model.hpp's constants) and the
                               period of the command timer (0.01): mass and dt_cmd finite and > 0, g finite                          */
    double kp[3], kv[3], ka[3]; /* position, velocity and attitude gains per axis: finite and >= 0                                    */
    double *x;              /* [B][9] in and out: the plant state                                                                     */
    const double *f_true;   /* [B][3] the true mass-normalised external force; it need not be what the planner was told               */
    const double *cmd;      /* [B][S][FRP_COMMAND_STRIDE] as frp_nmpc_command_batch wrote it                                          */
    const int *kind;        /* [B][S] FRP_COMMAND_*, as frp_nmpc_command_batch wrote it                                               */
    double *hold;           /* [B][FRP_VEHICLE_HOLD_STRIDE] in and out: the last published position and yaw                           */
    /* optional outputs, NULL: not written                                                                                            */
    double *trace;          /* [B][S][9] the state after every sample                                                                 */
    int *sat;               /* [B][S] FRP_VEHICLE_SAT_*                                                                                */
} frp_nmpc_vehicle;

/* S command samples flown by each of B vehicles, in ONE launch; sample s + 1 sees the state and the hold sample s left.  Per sample:
 *   setpoint    TRAJ, END: p_ref = cmd 0-2, v_ref = cmd 7-9, w_ff = cmd 10-12, a_ff = cmd 13-15, and the yaw of the published quaternion
 *               (x, y, z, w) = cmd 3-6, which cmdTrajCallback composes in X * Y * Z order: with R = Quaternion::toRotationMatrix, term by
 *               term, yaw_ref = atan2(-R01, R00) = atan2(-(2 y x - 2 z w), 1 - (2 y y + 2 z z)).
 *               YAW: p_ref = cmd 0-2, yaw_ref = cmd 12 (the yaw itself, as the timer stores it), everything else 0.
 *               Where one of these published: hold <- (p_ref, yaw_ref, 0, 0, 0, 0).
 *               NONE, NO_YAW_INPUT and any other value: p_ref = hold 0-2, yaw_ref = hold 3, everything else 0; hold stays.
 *   controller  a = a_ff + kp o (p_ref - p) + kv o (v_ref - v) + g e3;  T = clamp(mass |a|, thrust bounds);  zB = a / |a|, e3 where
 *               |a| == 0;  c = Rz(-yaw_ref) zB;  roll_d = asin(clamp(-c_y, +-1)), pitch_d = atan2(c_x, c_z) -- the inverse of the
 *               model's zB(roll, pitch, yaw_ref) --, both clamped to the attitude bounds;  w = clamp(w_ff + ka o ((roll_d, pitch_d,
 *               yaw_ref) - e), rate bounds), the yaw error d first moved into (-pi, pi]: d - 2 pi ceil((d - pi) / (2 pi)).
 *               Every bound is frp_model.hpp's lower_bound / upper_bound, the planner's own stage bounds: thrust 3, rates 0-2,
 *               roll and pitch 14-15.
 *   plant       n_sub Heun steps of h = dt_cmd / n_sub with (w, T) held:  k1 = f(x), k2 = f(x + h k1), x <- x + h / 2 (k1 + k2)  for
 *               p' = v, v' = accel(v, e, T, f_true) of frp_model.hpp, e' = w -- rk2() of that file at another step.
 * No contraction: every product and sum above is rounded on its own (the model's sincos carries its own fma chain).
 * FRP_ERR_ARG: v or any array other than trace and sat NULL, B < 1, S < 1, B * S beyond 2^31 - 1, n_sub outside [1, FRP_VEHICLE_MAX_SUB],
 * mass or dt_cmd not finite and positive, g not finite, a gain negative or not finite. */
int frp_nmpc_vehicle_step(const frp_nmpc_vehicle *v, void *stream);

/* Where mask[b] != 0 (mask == NULL: everywhere): x[b] <- x0[b] and hold[b] <- (x0 0-2, x0 8, 0, 0, 0, 0), the vehicle's own position
 * and yaw, so that a reset vehicle hovers until something is published.  Every other vehicle keeps both.
 * FRP_ERR_ARG: B < 1, x0, x or hold NULL. */
int frp_nmpc_vehicle_reset(int B, const double *x0, const int *mask, double *x, double *hold, void *stream);

/* The message of a plant state, msg [B][FRP_VEHICLE_MSG_STRIDE] from x [B][9]: position; the quaternion qz * qy * qx of eulerToRot
 * (Quaternion(cos(a / 2), sin(a / 2) axis) each, Eigen's scalar product, stored x y z w); the linear twist -- x 3-5 for FRP_ODOM_WORLD,
 * R(q)' x 3-5 for FRP_ODOM_BODY with R = Quaternion::toRotationMatrix of that quaternion --; the angular twist 0 (the plant state
 * carries none, and the callbacks read none).
 * FRP_ERR_ARG: B < 1, type neither FRP_ODOM_WORLD nor FRP_ODOM_BODY, x or msg NULL. */
int frp_nmpc_vehicle_message(int B, int type, const double *x, double *msg, void *stream);

/* odometryCallback (type FRP_ODOM_WORLD, :421-448) or odometryTransCallback (FRP_ODOM_BODY, :456-478) for B planners.  Where
 * fresh[b] != 0 (a message arrived for this planner):
 *   state_prev[b] <- state[b]                                   stateOdomPrevious_ = stateOdom_ (state_prev == NULL: not kept)
 *   state 0-2 <- msg 0-2
 *   state 3-5 <- msg 7-9 (WORLD), R(q) msg 7-9 (BODY)           q = (w, x, y, z) = msg 6, 3, 4, 5; R = Quaternion::toRotationMatrix
 *   state 6-8 <- getEulerAnglesFromQuaternion(q):  roll = atan2(2 (w x + y z), 1 - 2 (x x + y y)),  pitch = asin(2 (w y - z x)),
 *                yaw = atan2(2 (w z + x y), 1 - 2 (y y + z z))  -- as written, the argument of asin is not clamped
 *   have_odom[b] <- 1
 * Everywhere else state, state_prev and have_odom stay.  state [B][9] is the `state` of frp_nmpc_fsm_exec_in and frp_nmpc_tick_in,
 * have_odom the array of frp_nmpc_fsm.
 * FRP_ERR_ARG: B < 1, another type, msg, fresh, state or have_odom NULL. */
int frp_nmpc_vehicle_odometry(int B, int type, const double *msg, const int *fresh, double *state, double *state_prev, int *have_odom,
                              void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_VEHICLE_H */
