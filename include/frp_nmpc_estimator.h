/* frp_nmpc.h section (13), frp_nmpc_estimator.h: the force estimator on the device -- what the planner is TOLD about the external force,
 * made from what the vehicle flew.  With it the last arrow of a simulated fleet's period stays in device memory: commands -> plant (under
 * f_true) -> thrust and measurements -> estimate -> frp_nmpc_fsm_force -> replan, period after period in one captured graph.  frp_nmpc.h
 * includes it, and including it alone works too (it pulls in frp_nmpc.h for the error codes and frp_nmpc_vehicle, and carries its own
 * extern "C").  Same ABI version: no existing struct changed, and a library without these three symbols is refused by the loaders that
 * need them (solver.ESTIMATOR_EXPORTS).
 *
 * NO REFERENCE COUNTERPART.  The reference has no estimator in its tree: extforceCallback (plan_manage/src/nmpc_manage.cpp:366-418)
 * subscribes to a WrenchStamped that another node publishes.  What is specified here is a velocity-residual (momentum) observer on the
 * planner's OWN model -- csrc/frp_model.hpp's accel() with a zero force vector, called, not re-derived --, so this layer is
 * STRUCTURALLY UNPINNED: no test vector of the reference reaches it.  tests/estimator_oracle.py is the executable statement;
 * tests/golden/estimator_mp.npz the same discrete scheme in 50 digits.
 * The measurements are whatever the caller hands in: from frp_nmpc_vehicle_step's trace they are the TRUE plant state.  Noise, bias and
 * delay of a real odometry are the caller's to add (or to bring, with a real fleet's odometry in `meas`).
 *
 * Every call: every pointer is DEVICE memory, asynchronous on `stream`, nothing allocated, nothing read back, capturable into a
 * hipGraph with the tick; one launch, one thread per vehicle, 256 per workgroup, no kernel waits on another workgroup.  FRP_ERR_ARG
 * before any device call, FRP_ERR_NO_DEVICE without a device. */
#ifndef FRP_NMPC_ESTIMATOR_H
#define FRP_NMPC_ESTIMATOR_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

/* status[b][s]: what the update did with sample s */
#define FRP_EST_SKIPPED 0  /* an input was not finite: nothing absorbed, the next finite sample starts over       */
#define FRP_EST_FIRST 1    /* no previous measurement: kept as one, nothing absorbed                               */
#define FRP_EST_ABSORBED 2 /* one residual went into the filter                                                    */

/* frp_nmpc_vehicle_step, and in addition thrust[b][s] <- the clamped collective thrust T that sample s was flown with (the T of that
 * call's controller, after the thrust bounds): what an estimator needs beside the states.  x, hold, trace and sat are what
 * frp_nmpc_vehicle_step writes, to the bit (the same kernel text; frp_nmpc_vehicle_step launches the instantiation without the store).
 * thrust [B][S], device.  FRP_ERR_ARG: thrust NULL, and whatever frp_nmpc_vehicle_step refuses.
 * (v is a const frp_nmpc_vehicle *, written with its struct tag: where frp_nmpc_vehicle.h is the file a program includes, frp_nmpc.h
 * reaches this header before that one's struct.) */
struct frp_nmpc_vehicle;
int frp_nmpc_vehicle_step_observed(const struct frp_nmpc_vehicle *v, double *thrust, void *stream);

typedef struct frp_nmpc_estimator {
    int B, S, min_samples;     /* vehicles, samples per call (>= 1), residuals before the estimate counts as fresh (>= 1)             */
    double dt, alpha;          /* the sample period (the command timer's 0.01): finite and > 0; the filter gain in (0, 1]            */
    const double *meas;        /* [B][S][9] the state after each sample: frp_nmpc_vehicle.trace, or a real fleet's odometry          */
    const double *thrust;      /* [B][S] the thrust each sample was flown with: frp_nmpc_vehicle_step_observed's                      */
    double *f_hat;             /* [B][3] in and out: the estimate, mass-normalised                                                    */
    double *y_prev;            /* [B][9] in and out: the last measurement kept                                                        */
    int *count;                /* [B] in and out: -1 no previous measurement, k >= 0 residuals absorbed since (saturating at INT_MAX)  */
    double *force;             /* [B][3] out: the force of frp_nmpc_fsm_force                                                         */
    int *fresh;                /* [B] out: the fresh of frp_nmpc_fsm_force                                                            */
    /* optional outputs, NULL: not written                                                                                            */
    double *residual;          /* [B][S][3] the residual of every sample (0 where none was formed)                                    */
    int *status;               /* [B][S] FRP_EST_*                                                                                    */
} frp_nmpc_estimator;

/* S samples absorbed by each of B estimators, in ONE launch.  Per sample s, with y = meas[b][s] (v = y 3-5, e = y 6-8) and
 * T = thrust[b][s], the first of these that applies:
 *   not finite   any of the nine y or T is a NaN or an infinity: count <- -1, status FRP_EST_SKIPPED, residual 0; f_hat and y_prev stay
 *                -- a NaN never enters the filter, and the next finite sample starts over as a first one.
 *   first        count == -1: y_prev <- y, count <- 0, status FRP_EST_FIRST, residual 0; f_hat stays.
 *   update       a0 = accel(v_prev, e_prev, T, 0), a1 = accel(v, e, T, 0) with frp_model.hpp's accel_t and a zero force vector; per
 *                axis  dv = (v - v_prev) / dt,  m = 0.5 * (a0 + a1),  r = dv - m,  f_hat <- f_hat + alpha * (r - f_hat);
 *                count <- min(count + 1, INT_MAX), y_prev <- y, status FRP_EST_ABSORBED, residual r.
 *                r is the trapezoidal velocity residual: under a constant force f and a thrust held over the sample it is f up to the
 *                second order of dt.  The sines and cosines of a sample's end are the next sample's start: computed once.
 * After the S samples: force[b] <- f_hat, fresh[b] <- (count >= min_samples).
 * No contraction: every product, quotient and sum above is rounded on its own, in the order written (the model's sincos carries its own
 * fma chain).
 * FRP_ERR_ARG: e or any array other than residual and status NULL, B < 1, S < 1, B * S beyond 2^31 - 1, min_samples < 1, dt not finite
 * and positive, alpha a NaN or outside (0, 1]. */
int frp_nmpc_estimator_update(const frp_nmpc_estimator *e, void *stream);

/* Where mask[b] != 0 (mask == NULL: everywhere): f_hat[b] <- 0, count[b] <- -1, force[b] <- 0, fresh[b] <- 0.  y_prev and every other
 * estimator stay (count == -1 makes y_prev unread).
 * FRP_ERR_ARG: B < 1, f_hat, y_prev, count, force or fresh NULL. */
int frp_nmpc_estimator_reset(int B, const int *mask, double *f_hat, double *y_prev, int *count, double *force, int *fresh, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_ESTIMATOR_H */
