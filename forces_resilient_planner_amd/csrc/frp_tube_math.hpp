// frp_tube_math.hpp -- the per-lane arithmetic of the tube kernel (frp_tube.hip): everything a lane computes between reading
// a plan row and handing its results to the wave.  It is `__host__ __device__` so that tests/cpp/tube_harness.cpp compiles
// THIS text with a plain C++ compiler (where the HIP attributes are defined away) and the CPU suite compares it with the
// multiprecision fixture tests/golden/tube_mp.npz: the kernel and the harness call the same build_phi, phi_norm1, tube_panels,
// tube_lane and sqrt_sym3, and there is one copy of each.  Method and accuracy: see the header comment of frp_tube.hip.
#pragma once
#include <math.h>
#include "../../include/frp_nmpc.h"

#if defined(__HIPCC__)
#define FRP_TB_FN __host__ __device__
#define FRP_TB_CONST __device__ constexpr
#else
#define FRP_TB_FN
#define FRP_TB_CONST constexpr
#ifndef __forceinline__
#define __forceinline__ inline __attribute__((always_inline))
#endif
#endif

#define FRP_TB_NOINLINE __attribute__((noinline))

namespace frp {

#ifndef FRP_TB_GSTEPS
#define FRP_TB_GSTEPS 2
#define FRP_TB_GTERMS 24
#endif
constexpr int TB_NZ = 17, TB_SYM = 45, TB_STAGES_PER_WAVE = 21, TB_TAYLOR = 14, TB_GSTEPS = FRP_TB_GSTEPS, TB_GTERMS = FRP_TB_GTERMS;

// The domain of one quadrature panel, in nu = ||Phi||_1 t (phi_norm1 below).  Measured with tests/cpp/tube_harness against the
// 50-digit fixture (frp_tube.hip's header comment has the table): one panel keeps a stage's Qd to 6e-14 for nu < 6 and loses
// two decades in [6, 8); 5 leaves a factor (6/5)^16 ~ 18 of the 8-node rule's error to that edge, and every plan inside the
// stage bounds at Ts <= 0.1 (nu <= 4.6) still has one panel.
constexpr double TB_NU0 = 5.0;
constexpr int TB_MAX_PANELS = FRP_TUBE_MAX_PANELS, TB_JACOBI_SWEEPS = 8;

// K rows 0..2 (nmpc_solver.cpp:28-30); row 3 = [0 0 -8 0 0 -6 0 0 0] (:31) is folded into PhiS::b8 / m3.
#define TB_K(a, j) (tb_gain[(a) * 9 + (j)])
FRP_TB_CONST double tb_gain[27] = {-2.0, 5.0, 0.0, -1.0, 4.0, 0.0, -8.0, 0.0, 0.0,
                                   -5.0, -2.0, 0.0, -4.0, -1.0, 0.0, 0.0, -8.0, 0.0,
                                   -2.0, -2.0, 0.0, -1.0, -1.0, 0.0, 0.0, 0.0, -8.0};
FRP_TB_CONST double tb_glx[8] = {-0.9602898564975362, -0.7966664774136267, -0.525532409916329, -0.18343464249564978,
                                 0.18343464249564978, 0.525532409916329,   0.7966664774136267, 0.9602898564975362};
FRP_TB_CONST double tb_glw[8] = {0.10122853629037669, 0.22238103445337434, 0.31370664587788705, 0.36268378337836177,
                                 0.36268378337836177, 0.31370664587788705, 0.22238103445337434, 0.10122853629037669};

struct PhiS {          // the variable rows 3..5 of Phi = A + B K
    double b8[3];      // column 2:  -8 * B(3+a, 3)
    double m3[3][3];   // columns 3..5: R drag R' with -6 * B(3+a, 3) added to column 5
    double m6[3][3];   // columns 6..8: d a / d (roll, pitch, yaw)
};

FRP_TB_FN __forceinline__ int sym_index(int m, int n) { return m * 9 - (m * (m - 1)) / 2 + (n - m); } // m <= n

// updateMatrix (:615-699) + eulerToRot (:554-565); R out row-major
FRP_TB_FN inline void build_phi(const double *z, double mass, double drag, PhiS &P, double R[9])
{
    const double thrust = z[3], v1 = z[11], v2 = z[12], v3 = z[13], roll = z[14], pitch = z[15], yaw = z[16];
    double sr, cr, sp, cp, sy, cy;
    sincos(roll, &sr, &cr); sincos(pitch, &sp, &cp); sincos(yaw, &sy, &cy);
    const double c0 = thrust / mass;
    const double c5 = cp * sp, c6 = cp * sr, c7 = cp * cr, c8 = sp * cr, c9 = sp * sr;
    const double c1 = cr * sy - c9 * cy, c2 = sr * cy - c8 * sy, c3 = cr * cy + c9 * sy, c4 = sr * sy + c8 * cy;
    // R = Rz Ry Rx
    R[0] = cy * cp; R[1] = cy * c9 - sy * cr; R[2] = cy * c8 + sy * sr;
    R[3] = sy * cp; R[4] = sy * c9 + cy * cr; R[5] = sy * c8 - cy * sr;
    R[6] = -sp;     R[7] = c6;                R[8] = c7;
    const double t10 = c6 * c4 - c7 * c1, t11 = c3 * c4 + c1 * c2, t12 = c6 * c2 - c7 * c3;
    P.m6[0][0] = c0 * c1 + drag * (v3 * t10 + v2 * t11 - 2 * v1 * c4 * c1);
    P.m6[1][0] = -c0 * c3 + drag * (v1 * t11 - v3 * t12 - 2 * v2 * c3 * c2);
    P.m6[2][0] = -c0 * c6 + drag * (v1 * t10 - v2 * t12 + 2 * v3 * c7 * c6);
    const double sr2 = sr * sr, cp2 = cp * cp, sp2 = sp * sp;
    const double t20 = cy * (sp2 - cp2 + cp2 * sr2) + c9 * c1;
    const double t21 = 2 * c5 * cy * sy - c6 * (cy * c3 + sy * c1);
    const double t22 = sy * (cp2 - sp2 - cp2 * sr2) + c9 * c3;
    P.m6[0][1] = c0 * c7 * cy + drag * (v3 * t20 - v2 * t21 - v1 * 2 * (c5 * cy * cy + c6 * c1 * cy));
    P.m6[1][1] = c0 * c7 * sy - drag * (v3 * t22 - v1 * t21 - v2 * 2 * (c5 * sy * sy - c6 * c3 * sy));
    P.m6[2][1] = -c0 * c8 + drag * (v1 * t20 - v2 * t22 + v3 * 2 * (c5 - c5 * sr2));
    const double t30 = 2 * drag * (c3 * c1 - cp2 * cy * sy), t31 = drag * (c6 * c3 - c5 * sy);
    const double t32 = drag * (c3 * c3 - c1 * c1 - cp2 * cy * cy + cp2 * sy * sy), t33 = drag * (c6 * c1 + c5 * cy);
    P.m6[0][2] = c0 * c2 + v1 * t30 - v3 * t31 - v2 * t32;
    P.m6[1][2] = c0 * c4 - v1 * t32 - v3 * t33 - v2 * t30;
    P.m6[2][2] = -v2 * t33 - v1 * t31;
    // R diag(drag, drag, 0) R'
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) P.m3[a][c] = drag * (R[3 * a] * R[3 * c] + R[3 * a + 1] * R[3 * c + 1]);
    const double bt[3] = {c4 / mass, -c2 / mass, c7 / mass}; // Bt_(3..5, 3) (:692-694)
#pragma unroll
    for (int a = 0; a < 3; ++a) { P.b8[a] = -8.0 * bt[a]; P.m3[a][2] += -6.0 * bt[a]; }
}

FRP_TB_FN __forceinline__ void phi_mul(const PhiS &P, const double v[9], double o[9])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = v[3 + a];
        double s = P.b8[a] * v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) s += P.m3[a][c] * v[3 + c] + P.m6[a][c] * v[6 + c];
        o[3 + a] = s;
        double g = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) if (TB_K(a, j) != 0.0) g += TB_K(a, j) * v[j];
        o[6 + a] = g;
    }
}

FRP_TB_FN __forceinline__ void phiT_mul(const PhiS &P, const double v[9], double o[9])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double s0 = 0.0, s3 = v[c], s6 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (TB_K(a, c) != 0.0) s0 += TB_K(a, c) * v[6 + a];
            s3 += P.m3[a][c] * v[3 + a];
            if (TB_K(a, 3 + c) != 0.0) s3 += TB_K(a, 3 + c) * v[6 + a];
            s6 += P.m6[a][c] * v[3 + a];
            if (TB_K(a, 6 + c) != 0.0) s6 += TB_K(a, 6 + c) * v[6 + a];
        }
        if (c == 2) s0 += P.b8[0] * v[3] + P.b8[1] * v[4] + P.b8[2] * v[5];
        o[c] = s0; o[3 + c] = s3; o[6 + c] = s6;
    }
}

// v <- exp(h Phi) v  (TRANSPOSED: exp(h Phi') v): the TERMS-term series in Horner form,
// v + h Phi (v + h/2 Phi (v + h/3 Phi (...))) -- one product with Phi and nine multiply-adds per term (round 5; the term-by-term sum
// cost a scaling and an addition per entry on top: 0.20 -> 0.18 ms per 4096 planners, same values to rounding)
template <bool TRANSPOSED, int TERMS = TB_TAYLOR>
FRP_TB_FN __forceinline__ void expm_step(const PhiS &P, double h, double v[9])
{
    double y[9], nxt[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) y[j] = v[j];
    for (int n = TERMS; n >= 1; --n) {
        if (TRANSPOSED) phiT_mul(P, y, nxt); else phi_mul(P, y, nxt);
        const double f = h / (double)n;
#pragma unroll
        for (int j = 0; j < 9; ++j) y[j] = __builtin_fma(f, nxt[j], v[j]);
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = y[j];
}

// ||Phi||_1, the largest absolute column sum: rows 0..2 are [0 I 0], rows 3..5 are PhiS, rows 6..8 the gain rows
FRP_TB_FN inline double phi_norm1(const PhiS &P)
{
    double best = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        double s = (j >= 3 && j < 6) ? 1.0 : 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s += fabs(TB_K(a, j));
            s += j == 2 ? fabs(P.b8[a]) : (j < 3 ? 0.0 : (j < 6 ? fabs(P.m3[a][j - 3]) : fabs(P.m6[a][j - 6])));
        }
        best = s > best ? s : best;
    }
    return best;
}

// panels of [0, t] for a stage with nu = ||Phi||_1 t: ceil(nu / TB_NU0), at most TB_MAX_PANELS.  0 = outside the domain
// (nu beyond TB_MAX_PANELS * TB_NU0, or not a number): the caller marks the planner's output instead of losing digits silently
FRP_TB_FN inline int tube_panels(double nu)
{
    if (nu <= TB_NU0) return 1;
    if (!(nu <= TB_NU0 * TB_MAX_PANELS)) return 0;
    const int n = (int)ceil(nu / TB_NU0);
    return n < TB_MAX_PANELS ? n : TB_MAX_PANELS;
}

// One (stage, channel) of the kernel: row ch of exp(Phi t) -> g[0..8], then X += int_0^t (e^{-Phi s} d)(e^{-Phi s} d)' ds for
// d = e_{3+ch} (packed upper triangle).  tube_lane_one is the ONE-panel form: TB_GSTEPS TB_GTERMS-term steps for the row, 8-node
// Gauss-Legendre on [0, t] with the vector stepped from node to node by the TB_TAYLOR-term series.
// CODE GENERATION.  One panel is every stage of a plan inside the stage bounds, i.e. the whole hot path.  With the panel loop
// rolled around this text (one form for any number of panels) the MI355X gave E within 5.6e-16 of, but not bit-identical to, the
// kernel without panels, at the same speed.  Standing alone in the kernel this text compiles with both loops fully unrolled (eight
// copies of the node step); the pragmas ask for that here as well, and the many-panel form is a function of its own, called on
// copies of its operands, because inlined next to this one the compiler merges the two into the rolled form.  Cost in the kernel:
// 256 VGPRs with 5 spilled and 640 B of scratch per lane (230 / 0 / 0 without panels).  NOT YET MEASURED on the GPU in this
// form: that the bits of the one-panel stages equal those of the kernel without panels, and the time.
FRP_TB_FN __forceinline__ void tube_lane_one(const PhiS &P, double t, int ch, double *g, double X[TB_SYM])
{
    double v[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = (j == ch) ? 1.0 : 0.0;
#pragma unroll
    for (int n = 0; n < TB_GSTEPS; ++n) expm_step<true, TB_GTERMS>(P, t / TB_GSTEPS, v);
#pragma unroll
    for (int j = 0; j < 9; ++j) { g[j] = v[j]; v[j] = (j == 3 + ch) ? 1.0 : 0.0; }
    double s_prev = 0.0;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const double s = 0.5 * t * (1.0 + tb_glx[n]);
        expm_step<false>(P, -(s - s_prev), v);
        s_prev = s;
        const double wgt = 0.5 * t * tb_glw[n];
        int e = 0;
#pragma unroll
        for (int m = 0; m < 9; ++m)
#pragma unroll
            for (int nn = m; nn < 9; ++nn) X[e++] += wgt * v[m] * v[nn];
    }
}

// the same on `panels` > 1 equal panels: TB_GSTEPS steps of the row per panel, the node steps run on across the panel ends
FRP_TB_FN FRP_TB_NOINLINE void tube_lane_n(const PhiS &P, double t, int panels, int ch, double *g, double X[TB_SYM])
{
    double v[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = (j == ch) ? 1.0 : 0.0;
    const double h = t / (TB_GSTEPS * panels);
    for (int n = 0; n < TB_GSTEPS * panels; ++n) expm_step<true, TB_GTERMS>(P, h, v);
#pragma unroll
    for (int j = 0; j < 9; ++j) { g[j] = v[j]; v[j] = (j == 3 + ch) ? 1.0 : 0.0; }
    const double tp = t / (double)panels;
    double s_prev = 0.0;
    for (int pnl = 0; pnl < panels; ++pnl) {
        for (int n = 0; n < 8; ++n) {
            const double s = 0.5 * tp * (1.0 + tb_glx[n]);
            expm_step<false>(P, -(s - s_prev), v);
            s_prev = s;
            const double wgt = 0.5 * tp * tb_glw[n];
            int e = 0;
#pragma unroll
            for (int m = 0; m < 9; ++m)
#pragma unroll
                for (int nn = m; nn < 9; ++nn) X[e++] += wgt * v[m] * v[nn];
        }
        s_prev -= tp; // the next panel's nodes are measured from its own start
    }
}

FRP_TB_FN __forceinline__ void tube_lane(const PhiS &P, double t, int panels, int ch, double *g, double X[TB_SYM])
{
    if (panels == 1) {
        tube_lane_one(P, t, ch, g, X);
    } else { // on copies: operands whose address leaves the caller would live in memory for the one-panel form as well
        PhiS Pn = P;
        double gn[9], Xn[TB_SYM];
#pragma unroll
        for (int e = 0; e < TB_SYM; ++e) Xn[e] = 0.0;
        tube_lane_n(Pn, t, panels, ch, gn, Xn);
#pragma unroll
        for (int j = 0; j < 9; ++j) g[j] = gn[j];
#pragma unroll
        for (int e = 0; e < TB_SYM; ++e) X[e] += Xn[e];
    }
}

// principal square root of a symmetric positive definite 3x3 (q = xx xy xz yy yz zz), cyclic Jacobi; out row-major
FRP_TB_FN inline void sqrt_sym3(const double q[6], double E[9])
{
    double a00 = q[0], a01 = q[1], a02 = q[2], a11 = q[3], a12 = q[4], a22 = q[5];
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#define TB_ROT(app, aqq, apq, arp, arq, p, q_)                                                   \
    if (apq != 0.0) {                                                                            \
        const double th = (aqq - app) / (2.0 * apq);                                             \
        const double t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));                   \
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;                                     \
        app -= t * apq; aqq += t * apq; apq = 0.0;                                               \
        const double rp = arp, rq = arq;                                                         \
        arp = c * rp - s * rq; arq = s * rp + c * rq;                                            \
        _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                          \
            const double vp = V[i][p], vq = V[i][q_];                                            \
            V[i][p] = c * vp - s * vq; V[i][q_] = s * vp + c * vq;                               \
        }                                                                                        \
    }
    for (int sweep = 0; sweep < TB_JACOBI_SWEEPS; ++sweep) {
        TB_ROT(a00, a11, a01, a02, a12, 0, 1)
        TB_ROT(a00, a22, a02, a01, a12, 0, 2)
        TB_ROT(a11, a22, a12, a01, a02, 1, 2)
    }
#undef TB_ROT
    const double l[3] = {sqrt(fmax(a00, 0.0)), sqrt(fmax(a11, 0.0)), sqrt(fmax(a22, 0.0))};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) E[3 * i + j] = l[0] * V[i][0] * V[j][0] + l[1] * V[i][1] * V[j][1] + l[2] * V[i][2] * V[j][2];
}

} // namespace frp
