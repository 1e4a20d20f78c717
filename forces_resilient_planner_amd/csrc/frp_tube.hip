// frp_tube.hip -- SURVEY 8f row f-2: the tube (ego + disturbance ellipsoid) propagation that
// NMPCSolver::setFORCESParams runs for every stage before each NLP solve, batched on the device.  Its output, the
// per-stage matrices E_i, is the `ellipsoid` input of frp_nmpc_pack_batch (f-1), so plan -> tube -> pack -> solve
// stays in HBM.
//
// Reference (src/resilient_planner/plan_manage/src/nmpc_solver.cpp):
//   updateMatrix :615-699, eulerToRot :554-565, getDistrEllipsoid :567-611, setFORCESParams :484-521,
//   constants :11-31 (A/B/D pattern, K), :68-99 (mass, drag, ego size, noise bound), nmpc_utils.h:188-189.
//
// What the reference does per stage with Eigen -- two 9x9 complex Schur forms, three triangular Sylvester solves,
// four Pade matrix exponentials, a general 3x3 eigendecomposition -- is restated for a GPU lane through the
// quantities those calls define:
//   * the Sylvester solution of  Phi X + X Phi' = N - e^{-Phi t} N e^{-Phi' t},  N = t w^2 d d',  is the Gramian
//     X = t w^2 int_0^t (e^{-Phi s} d)(e^{-Phi s} d)' ds  (differentiate the integrand; the Gramian always solves
//     the equation, and the solution is unique unless two eigenvalues of Phi sum to zero).  The integrand is
//     entire, of exponential type 2 ||Phi||: 8-node Gauss-Legendre on a panel of length tp is exact to rounding while ||Phi|| tp
//     is small enough, and the vectors e^{-Phi s_j} d are stepped node to node with a 14-term Taylor series.  DOMAIN, measured
//     against the 50-digit fixture tests/golden/tube_mp.npz (tests/test_oracle_tube.py, this arithmetic compiled for the CPU):
//     with nu = ||Phi||_1 t (||Phi||_1 is 1.03 to 1.92 times ||Phi||_2 on the fixture), ONE panel gives the stage's Qd to 6e-14
//     of its largest entry for nu < 6, 5e-12 .. 8e-12 for 6 <= nu < 8, 7e-10 at 10 .. 14 and 2e-7 at 25 .. 30.  Plans inside the
//     stage bounds have nu 0.5 .. 2.3 at Ts = 0.05, up to 3.7 at 0.08 and 4.6 at 0.1; three times the thrust bound gives 5.3 at
//     0.05, 8.5 at 0.08, 30 at 0.3.  So [0, t] is split into ceil(nu / 5) equal panels per stage (TB_NU0; at most
//     FRP_TUBE_MAX_PANELS = 16), the node steps run on across the panel ends, and the fixture is met to 6e-14 (Qd) / 1.2e-13 (E)
//     at every Ts from 0.02 to 0.3 (nu up to 30, six panels; more panels than that are not compared with anything).  A stage with
//     nu > 80 (or not a number) is OUTSIDE the domain: the work stays bounded (16 panels) and every E of that planner is NaN --
//     never digits lost in silence.  frp_nmpc_tube_batch refuses a Ts at which a plan inside the stage bounds could get there;
//   * only rows 0..2 of e^{Phi t} are used (the position block): three Taylor-stepped vectors e^{Phi' t} e_j, two 24-term steps
//     per panel (the rows agree with the fixture to 4e-16 of their largest entry over the whole range);
//   * Phi is never formed densely: rows 0..2 are [0 I 0], rows 6..8 are the constant gain rows, so a product with
//     Phi or Phi' is 21 variable + 15 constant multiply-adds;
//   * sqrtm of the (symmetric positive definite) 3x3 sum by cyclic Jacobi, E = V sqrt(L) V'.
// Thread (stage k, channel i) owns disturbance channel i's Gramian and row i of e^{Phi t}; 21 stages per 64-lane
// wave, channels combined with wave shuffles (deterministic order).  The only sequential part -- the 9x9
// Minkowski recursion Q <- (1+1/beta) Q + (1+beta) Qd over the stages -- runs on 45 lanes afterwards.
//
// FP64 VALU-bound, not HBM-bound: 8*17*N bytes in and 72*N bytes out per problem against ~0.9 MFLOP.
// Deliberate deviations from two reference defects (uninitialised `temp` :573 -> 0; At_(5,8) accumulated across
// calls :689 -> fresh value) are documented in oracle/tube_oracle.py.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_tube_math.hpp"

namespace frp {

// LDS per stage: Qd (45) | G rows 0..2 of exp(Phi t) (27) | Q1 (6) | Q2 (6) | tr Qd (1)
constexpr int TS_QD = 0, TS_G = 45, TS_Q1 = 72, TS_Q2 = 78, TS_TR = 84, TS_STRIDE = 85;

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void tube_kernel(frp_nmpc_tube p)
{
    extern __shared__ double sm[];
    double *s_qo = sm + (size_t)p.N * TS_STRIDE; // 45: Q_origin of the running stage; afterwards 9 N outputs
    double *s_tmp = s_qo + (9 * p.N > TB_SYM ? 9 * p.N : TB_SYM); // 54: the products of the recursion's position block
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = wave * TB_STAGES_PER_WAVE + lane / 3, ch = lane % 3;
    const bool live = lane < 3 * TB_STAGES_PER_WAVE && k < p.N;
    const double *zb = p.mpc_output + (size_t)b * (p.N + 1) * TB_NZ;
    const double t = p.Ts;

    // ---- per (stage, channel): row ch of exp(Phi t), then the Gramian of channel ch ----------------------------
    double *st = sm + (size_t)(live ? k : 0) * TS_STRIDE;
    double X[TB_SYM];
#pragma unroll
    for (int e = 0; e < TB_SYM; ++e) X[e] = 0.0;
    double rootTr = 0.0;
    bool outside = false; // a stage of this planner lies outside the kernel's domain (see the header comment)
    if (live) {
        PhiS P;
        {
            double z[TB_NZ], R[9];
#pragma unroll
            for (int j = 0; j < TB_NZ; ++j) z[j] = zb[k * TB_NZ + j];
            build_phi(z, p.mass, p.drag, P, R);
            if (ch == 0) { // ego_size_ (:90-92), Q1 = R ego R' (:503)
                const double er = p.ego_r * p.ego_r, eh = p.ego_h * p.ego_h;
                int e = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int c = a; c < 3; ++c)
                        st[TS_Q1 + e++] = er * (R[3 * a] * R[3 * c] + R[3 * a + 1] * R[3 * c + 1]) + eh * R[3 * a + 2] * R[3 * c + 2];
            }
        }
        // panels of this stage's quadrature (and, times TB_GSTEPS, steps of its rows of exp(Phi t)) from nu = ||Phi||_1 t: one panel up to
        // TB_NU0, which covers every plan inside the stage bounds at Ts <= 0.1
        int panels = tube_panels(phi_norm1(P) * t);
        if (panels == 0) { outside = true; panels = TB_MAX_PANELS; } // bounded work for an absurd plan; its output is marked below
        tube_lane(P, t, panels, ch, st + TS_G + 9 * ch, X);
        const double scale = t * p.noise[ch] * p.noise[ch]; // N = t w^2 d d' (:591)
        double tr = 0.0;
#pragma unroll
        for (int m = 0; m < 9; ++m) tr += X[sym_index(m, m)];
        rootTr = sqrt(scale * tr);
        const double nrm = scale / rootTr;                  // X / sqrt(trace X) (:598)
#pragma unroll
        for (int e = 0; e < TB_SYM; ++e) X[e] *= nrm;
    }
    // combine the three channels of a stage (lanes 3s, 3s+1, 3s+2 of one wave): Qd = (sum sqrt tr)(sum X/sqrt tr)
    const int base = lane - ch;
    const double temp = __shfl(rootTr, base) + __shfl(rootTr, base + 1) + __shfl(rootTr, base + 2);
#pragma unroll
    for (int e = 0; e < TB_SYM; ++e) {
        const double q = temp * (__shfl(X[e], base) + __shfl(X[e], base + 1) + __shfl(X[e], base + 2));
        if (live && e % 3 == ch) st[TS_QD + e] = q;
    }
    if (live && ch == 0) st[TS_TR] = temp * temp; // tr Qd = temp * sum_i tr(X_i)/sqrt(tr X_i) = temp^2
    const int refused = __syncthreads_or(outside);

    // ---- the stage recursion of getDistrEllipsoid's Q_origin (:603-608), 45 lanes ------------------------------
    int em = 0, en = 0; // (row, col) of packed entry tid
    if (tid < TB_SYM) {
        int e = tid;
        while (e >= 9 - em) { e -= 9 - em; ++em; }
        en = em + e;
    }
    double qo = (tid < TB_SYM && em == en) ? p.epsilon * p.epsilon : 0.0; // Q_init (:487)
    double trQo = 9.0 * p.epsilon * p.epsilon;
    for (int s = 0; s < p.N; ++s) {
        const double *ss = sm + (size_t)s * TS_STRIDE;
        const double trd = ss[TS_TR];
        const double beta = sqrt(trQo / trd);
        const double ca = 1.0 + 1.0 / beta, cb = 1.0 + beta;
        if (tid < TB_SYM) { qo = ca * qo + cb * ss[TS_QD + tid]; s_qo[tid] = qo; }
        trQo = ca * trQo + cb * trd;
        __syncthreads();
        // position block of exp(Phi t) Q exp(Phi' t) (:605, :609): entry (a, c) = sum_m G[a][m] (sum_n Q[m][n] G[c][n]).  54 lanes take one
        // (entry, m) each and six add them up -- on six lanes alone the 9 x 9 sums were 250 instructions of every stage of this
        // sequential recursion, a quarter of the kernel (round 5: 0.188 -> 0.17 ms per 4096 planners)
        if (tid < 54) {
            const int pr = tid / 9, m = tid - 9 * pr;
            const int a = pr < 3 ? 0 : (pr < 5 ? 1 : 2), c = pr < 3 ? pr : (pr < 5 ? pr - 2 : 2);
            double row = 0.0;
#pragma unroll
            for (int n = 0; n < 9; ++n) row += s_qo[m <= n ? sym_index(m, n) : sym_index(n, m)] * ss[TS_G + 9 * c + n];
            s_tmp[tid] = ss[TS_G + 9 * a + m] * row;
        }
        __syncthreads();
        if (tid < 6) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < 9; ++m) acc += s_tmp[9 * tid + m];
            sm[(size_t)s * TS_STRIDE + TS_Q2 + tid] = acc;
        }
        __syncthreads();
    }

    // ---- per stage: Minkowski sum of ego and previous disturbance ellipsoid, square root (:503-513) -------------
    __syncthreads(); // s_qo is free now; the outputs leave through it so the global store is one contiguous run
    double *s_out = s_qo; // reuse: 9 N doubles (launcher sizes it)
    if (tid < p.N) {
        const double *ss = sm + (size_t)tid * TS_STRIDE;
        double q[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) q[e] = ss[TS_Q1 + e];
        if (tid > 0) {
            const double *q2 = ss - TS_STRIDE + TS_Q2;
            const double beta = sqrt((q[0] + q[3] + q[5]) / (q2[0] + q2[3] + q2[5]));
#pragma unroll
            for (int e = 0; e < 6; ++e) q[e] = (1.0 + 1.0 / beta) * q[e] + (1.0 + beta) * q2[e];
        }
        double E[9];
        sqrt_sym3(q, E);
#pragma unroll
        for (int j = 0; j < 9; ++j) s_out[9 * tid + j] = E[j];
    }
    __syncthreads();
    // a planner with a stage outside the domain gets NaN in every E: loud, where lost digits would be silent
    for (int e = tid; e < 9 * p.N; e += blockDim.x) p.ellipsoid[(size_t)b * 9 * p.N + e] = refused ? __builtin_nan("") : s_out[e];
}

} // namespace frp

extern "C" int frp_nmpc_tube_batch(const frp_nmpc_tube *p, void *stream)
{
    if (!p || p->B <= 0 || p->N < 1 || p->N > 64 || !p->mpc_output || !p->ellipsoid) return FRP_ERR_ARG;
    if (!(p->mass > 0.0) || !(p->Ts > 0.0) || !(p->epsilon > 0.0) || !(p->ego_r > 0.0) || !(p->ego_h > 0.0)) return FRP_ERR_ARG;
    for (int i = 0; i < 3; ++i) if (!(p->noise[i] > 0.0)) return FRP_ERR_ARG;
    // Ts so large that a plan INSIDE the stage bounds could leave the kernel's domain (include/frp_nmpc.h has the derivation): the
    // largest absolute column sum of Phi over those plans, column by column
    const double r3 = sqrt(3.0), dr = fabs(p->drag);
    double phi1 = fmax(9.0, 8.0 * r3 / p->mass);                                                              // columns 0, 1; 2
    phi1 = fmax(phi1, fmax(7.0 + r3 * dr, 1.0 + r3 * (dr + 6.0 / p->mass)));                                  // columns 3, 4; 5
    phi1 = fmax(phi1, 8.0 + r3 * (FRP_TUBE_THRUST_MAX / p->mass + 2.0 * dr * FRP_TUBE_SPEED_MAX));            // columns 6 .. 8
    if (!(p->Ts * phi1 <= frp::TB_NU0 * frp::TB_MAX_PANELS)) return FRP_ERR_ARG;
    const int waves = (p->N + frp::TB_STAGES_PER_WAVE - 1) / frp::TB_STAGES_PER_WAVE;
    const int tail = 9 * p->N > frp::TB_SYM ? 9 * p->N : frp::TB_SYM;
    const size_t lds = ((size_t)p->N * frp::TS_STRIDE + tail + 54) * sizeof(double);
    hipLaunchKernelGGL(frp::tube_kernel, dim3((unsigned)p->B), dim3(64 * waves), lds, static_cast<hipStream_t>(stream), *p);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}
