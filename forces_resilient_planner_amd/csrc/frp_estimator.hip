// frp_estimator.hip -- frp_nmpc.h section (13), frp_nmpc_estimator.h: the force estimator, a velocity-residual (momentum) observer on the
// planner's own dynamics.  No reference counterpart (the reference subscribes to a wrench another node publishes,
// plan_manage/src/nmpc_manage.cpp:366-418); tests/estimator_oracle.py is the executable statement.
//
//   * One thread per vehicle, 256 per workgroup, no LDS, no barrier, no atomics: an estimator reads and writes its own rows alone.  The
//     estimate, the previous measurement's velocity, its sines and cosines and the counter live in registers across the S samples; per
//     sample a thread reads 72 bytes of measurement and 8 of thrust and (where asked) writes 24 bytes of residual and a status.  Rows of
//     neighbouring lanes are S * 72 bytes apart, so the loads are not coalesced -- at 4096 vehicles and S = 5 that is 1.6 MB per call:
//     the cost is the launch.
//   * The model is frp_model.hpp's accel_t<false> with make_trig and a zero force vector: called, not re-derived.  The trig of a sample's
//     end is the next sample's start, computed once; a skipped or first sample leaves none, so the trig of y_prev is (re)computed where
//     an update finds none in registers (`have_trig`).
//   * No contraction in this file (the build passes -ffp-contract=off as well): the quotient, the mean, the residual and the filter step
//     are rounded one by one, as the header writes them; the model's sincos_bounded carries explicit fma calls, which stay.
//   * Every index is b < B and s < S as the entry point checked them (B * S fits an int; offsets are formed in size_t).
//   * Every store is a plain C++ store from a vector lane; no inline assembly.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_model.hpp"
#include "frp_fleet.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace estimator {

using namespace fleet;

constexpr int NXV = FRP_VEHICLE_STATE;

__global__ __launch_bounds__(THREADS) void update_kernel(frp_nmpc_estimator c)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= c.B) return;
    const int S = c.S;
    const double zero[3] = {0.0, 0.0, 0.0};
    double fh[3], yp[NXV];
#pragma unroll
    for (int i = 0; i < 3; i++) fh[i] = c.f_hat[(size_t)b * 3 + i];
#pragma unroll
    for (int i = 0; i < NXV; i++) yp[i] = c.y_prev[(size_t)b * NXV + i];
    int count = c.count[b];
    Trig tp = {0.0, 1.0, 0.0, 1.0, 0.0, 1.0};
    bool have_trig = false; // tp holds the sines and cosines of yp 6-8
    for (int s = 0; s < S; s++) {
        const double *row = c.meas + ((size_t)b * S + s) * NXV;
        double y[NXV];
#pragma unroll
        for (int i = 0; i < NXV; i++) y[i] = row[i];
        const double T = c.thrust[(size_t)b * S + s];
        bool ok = finite_d(T);
#pragma unroll
        for (int i = 0; i < NXV; i++) ok = ok && finite_d(y[i]);
        double r[3] = {0.0, 0.0, 0.0};
        int status;
        if (!ok) {
            count = -1;
            have_trig = false;
            status = FRP_EST_SKIPPED;
        } else if (count == -1) {
#pragma unroll
            for (int i = 0; i < NXV; i++) yp[i] = y[i];
            count = 0;
            have_trig = false;
            status = FRP_EST_FIRST;
        } else {
            if (!have_trig) tp = make_trig(yp + 6);
            const Trig tn = make_trig(y + 6);
            double a0[3], a1[3];
            accel_t<false>(yp + 3, tp, T, zero, a0, nullptr);
            accel_t<false>(y + 3, tn, T, zero, a1, nullptr);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double dv = (y[3 + i] - yp[3 + i]) / c.dt;
                const double m = 0.5 * (a0[i] + a1[i]);
                r[i] = dv - m;
                fh[i] = fh[i] + c.alpha * (r[i] - fh[i]);
            }
            count = count < INT_MAX ? count + 1 : INT_MAX;
#pragma unroll
            for (int i = 0; i < NXV; i++) yp[i] = y[i];
            tp = tn;
            have_trig = true;
            status = FRP_EST_ABSORBED;
        }
        if (c.residual) {
#pragma unroll
            for (int i = 0; i < 3; i++) c.residual[((size_t)b * S + s) * 3 + i] = r[i];
        }
        if (c.status) c.status[(size_t)b * S + s] = status;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        c.f_hat[(size_t)b * 3 + i] = fh[i];
        c.force[(size_t)b * 3 + i] = fh[i];
    }
#pragma unroll
    for (int i = 0; i < NXV; i++) c.y_prev[(size_t)b * NXV + i] = yp[i];
    c.count[b] = count;
    c.fresh[b] = count >= c.min_samples ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void reset_kernel(int B, const int *mask, double *f_hat, int *count, double *force, int *fresh)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    if (mask && mask[b] == 0) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        f_hat[(size_t)b * 3 + i] = 0.0;
        force[(size_t)b * 3 + i] = 0.0;
    }
    count[b] = -1;
    fresh[b] = 0;
}

} // namespace estimator
} // namespace frp

extern "C" {

int frp_nmpc_estimator_update(const frp_nmpc_estimator *e, void *stream)
{
    using namespace frp::estimator;
    if (!e || e->B < 1 || e->S < 1 || (long long)e->B * e->S > 0x7fffffffLL || e->min_samples < 1) return FRP_ERR_ARG;
    if (!positive(e->dt) || !(e->alpha > 0.0 && e->alpha <= 1.0)) return FRP_ERR_ARG;
    if (!e->meas || !e->thrust || !e->f_hat || !e->y_prev || !e->count || !e->force || !e->fresh) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(update_kernel, blocks_for(e->B), stream, *e);
}

int frp_nmpc_estimator_reset(int B, const int *mask, double *f_hat, double *y_prev, int *count, double *force, int *fresh, void *stream)
{
    using namespace frp::estimator;
    if (B < 1 || !f_hat || !y_prev || !count || !force || !fresh) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(reset_kernel, blocks_for(B), stream, B, mask, f_hat, count, force, fresh);
}

} // extern "C"
