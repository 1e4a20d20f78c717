/*
 * nmpc_ipm.c -- TEST INFRASTRUCTURE (see nmpc_oracle.h): CPU FP64 interior-point solver for the
 * reference NLP (matlab_code/setup.m:36-66, mpc/normal/mpc_generator_normal.m:1-50):
 *
 *   min  sum_k f_k(z_k, p_k)
 *   s.t. x_0 = xinit,  [x_{k+1}; w_{k+1}] = c(z_k, p_k)  (k = 0..N-2),
 *        lb <= z_k <= ub,  A_k pos_k - b_k <= 1e-5.
 *
 * It stands in for the reference's closed ForcesPro binary (licence-locked: "parity unpinned" at
 * the solver level, see nmpc_oracle.h).  Method: primal-dual interior point with Mehrotra
 * predictor-corrector; the stage Hessian is the exact (constant) cost Hessian -- a Gauss-Newton
 * Hessian of the Lagrangian, the reference uses per-stage BFGS instead -- and the
 * Newton KKT system is solved by a block-structured Riccati recursion over the stage chain
 * (state s = [w; x], 13, control u, 4).  The HIP product implements the same iteration, so the two
 * can be compared iterate by iterate.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "nmpc_oracle.h"
#ifdef ORC_TRACE
#include <stdio.h>
#endif

void orc_rk2(const double *x, const double *u, const double *fext, double *xn, double *Ax, double *Bx);
void orc_cost_quadratic(const double *p, int stage_class, int model, double *hd, double *hc, double *q, double *cst);
void orc_rk2_hess(const double *x, const double *u, const double *fext, const double *yp, const double *yv, double *H);

#define NS 13
#define HU_OFF 1e-5 /* hu = 1e-5, mpc_generator_normal.m:14 */
#define S_MIN 1e-2
#define MU_FLOOR_FRAC 0.3
#define THETA_DOWN 0.25
#define THETA_UP 0.1
#define KAPPA_LAM 2.0      /* multiplier safeguard: s_i lam_i >= mu / KAPPA_LAM after every step */
#define DIVERGE_RS 1e12
#define EXACT_SWITCH_EQ 1e-1

void orc_default_options(orc_options *o)
{
    o->maxit = 200;
    o->tol_stat = 1e-4;
    o->tol_eq = 1e-4;
    o->tol_ineq = 1e-4;
    o->tol_comp = 1e-4;
    o->mu0 = 1.0;
    o->ftb = 0.99;
    o->hessian = ORC_HESSIAN_DEFAULT;
    o->diverge_mu = 1e3;
    o->twist = 0;
}

typedef struct {
    /* model linearisation */
    double Ax[81], Bx[36], d[NS]; /* d = prev(z_{k}) - s_{k+1}, s-order [w;x]; stored on stage k   */
    double hd[17], hc, q[17];      /* cost 1/2 z'Hz + q'z                                           */
    /* factorisation */
    double L[16], Kt[4 * NS], kt[4], P[NS * NS], p[NS], Pd[NS];
    double phi[17];                /* rhs gradient of the current solve                             */
    double PhiD[17], PhiPos[9];    /* barrier-augmented Hessian: diagonal + pos 3x3 block           */
    double Hd[100];                /* exact Hessian of y'c(z) over (rates, T, v, e), see orc_rk2_hess  */
    int useH;
    double thetaH; /* weight of the dynamics Hessian */
} stage_ws;

static int stage_class_of(int k, int N) { return k == 0 ? ORC_STAGE_FIRST : (k == N - 1 ? ORC_STAGE_LAST : ORC_STAGE_MID); }

/* Backward Riccati step for stage k given (Pn, pn) of stage k+1 (NULL on the last stage).
 * full != 0: factorise (L, Kt, P, Pd) and the vector part; full == 0: vector part only (kt, p). */
static int riccati_step(stage_ws *w, const double *Pn, const double *pn, int full)
{
    double Q[17 * 17], q[17];
    const double *Ax = w->Ax, *Bx = w->Bx;
    memcpy(q, w->phi, sizeof q);
    if (pn) {
        double h[NS];
        if (full) {
            for (int i = 0; i < NS; i++) {
                double a = 0;
                for (int j = 0; j < NS; j++) a += Pn[i * NS + j] * w->d[j];
                w->Pd[i] = a;
            }
        }
        for (int i = 0; i < NS; i++) h[i] = w->Pd[i] + pn[i];
        for (int j = 0; j < 4; j++) {
            double a = h[j];
            for (int i = 0; i < 9; i++) a += Bx[i * 4 + j] * h[4 + i];
            q[j] += a;
        }
        for (int j = 0; j < 9; j++) {
            double a = 0;
            for (int i = 0; i < 9; i++) a += Ax[i * 9 + j] * h[4 + i];
            q[8 + j] += a;
        }
    }
    if (full) {
        memset(Q, 0, sizeof Q);
        for (int i = 0; i < 17; i++) Q[i * 17 + i] = w->PhiD[i];
        for (int i = 0; i < 4; i++) Q[i * 17 + 4 + i] = Q[(4 + i) * 17 + i] = w->hc;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Q[(8 + i) * 17 + 8 + j] += w->PhiPos[i * 3 + j];
        if (w->useH) {
            static const int zi[10] = {0, 1, 2, 3, 11, 12, 13, 14, 15, 16};
            for (int i = 0; i < 10; i++)
                for (int j = 0; j < 10; j++) Q[zi[i] * 17 + zi[j]] += w->thetaH * w->Hd[i * 10 + j];
        }
        if (Pn) {
            /* M = [I4 0 0; Bx 0 Ax] (rows [w;x] of stage k+1, cols [u w x] of stage k) */
            double PxxA[81], PxxB[36], T[36]; /* T = Pwx + Bx'Pxx  (4x9) */
            for (int i = 0; i < 9; i++) {
                for (int j = 0; j < 9; j++) {
                    double a = 0;
                    for (int l = 0; l < 9; l++) a += Pn[(4 + i) * NS + 4 + l] * Ax[l * 9 + j];
                    PxxA[i * 9 + j] = a;
                }
                for (int j = 0; j < 4; j++) {
                    double a = 0;
                    for (int l = 0; l < 9; l++) a += Pn[(4 + i) * NS + 4 + l] * Bx[l * 4 + j];
                    PxxB[i * 4 + j] = a;
                }
            }
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 9; j++) T[i * 9 + j] = Pn[i * NS + 4 + j] + PxxB[j * 4 + i];
            /* Quu += Pww + Pwx Bx + Bx' Pxw + Bx' Pxx Bx */
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) {
                    double a = Pn[i * NS + j];
                    for (int l = 0; l < 9; l++) a += T[i * 9 + l] * Bx[l * 4 + j] + Bx[l * 4 + i] * Pn[(4 + l) * NS + j];
                    Q[i * 17 + j] += a;
                }
            /* Qux += T Ax */
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 9; j++) {
                    double a = 0;
                    for (int l = 0; l < 9; l++) a += T[i * 9 + l] * Ax[l * 9 + j];
                    Q[i * 17 + 8 + j] += a;
                    Q[(8 + j) * 17 + i] += a;
                }
            /* Qxx += Ax' Pxx Ax */
            for (int i = 0; i < 9; i++)
                for (int j = 0; j < 9; j++) {
                    double a = 0;
                    for (int l = 0; l < 9; l++) a += Ax[l * 9 + i] * PxxA[l * 9 + j];
                    Q[(8 + i) * 17 + 8 + j] += a;
                }
        }
#ifdef ORC_TRACE
        fprintf(stderr, "orc Quu %.9e %.9e %.9e %.9e | %.6e %.6e %.6e %.6e %.6e %.6e\n", Q[0], Q[18], Q[36], Q[54], Q[17], Q[34], Q[35], Q[51], Q[52], Q[53]);
#endif
        /* Cholesky of Quu */
        double *L = w->L;
        memset(L, 0, 16 * sizeof(double));
        for (int j = 0; j < 4; j++) {
            double dsum = Q[j * 17 + j];
            for (int l = 0; l < j; l++) dsum -= L[j * 4 + l] * L[j * 4 + l];
            if (!(dsum > 0.0)) return -1;
            const double dj = sqrt(dsum);
            L[j * 4 + j] = dj;
            for (int i = j + 1; i < 4; i++) {
                double a = Q[i * 17 + j];
                for (int l = 0; l < j; l++) a -= L[i * 4 + l] * L[j * 4 + l];
                L[i * 4 + j] = a / dj;
            }
        }
        /* Kt = L^-1 Qus (4 x 13) */
        for (int c = 0; c < NS; c++)
            for (int i = 0; i < 4; i++) {
                double a = Q[i * 17 + 4 + c];
                for (int l = 0; l < i; l++) a -= L[i * 4 + l] * w->Kt[l * NS + c];
                w->Kt[i * NS + c] = a / L[i * 4 + i];
            }
        for (int i = 0; i < NS; i++)
            for (int j = 0; j < NS; j++) {
                double a = Q[(4 + i) * 17 + 4 + j];
                for (int l = 0; l < 4; l++) a -= w->Kt[l * NS + i] * w->Kt[l * NS + j];
                w->P[i * NS + j] = a;
            }
    }
    for (int i = 0; i < 4; i++) {
        double a = q[i];
        for (int l = 0; l < i; l++) a -= w->L[i * 4 + l] * w->kt[l];
        w->kt[i] = a / w->L[i * 4 + i];
    }
    for (int i = 0; i < NS; i++) {
        double a = q[4 + i];
        for (int l = 0; l < 4; l++) a -= w->Kt[l * NS + i] * w->kt[l];
        w->p[i] = a;
    }
    return 0;
}

typedef struct {
    int N, M, mc; /* mc = 34 + M constraint slots per stage */
    stage_ws *st;
    double *z, *y, *ynew, *dz;        /* [N*17], [N*13] (s-order), [N*13], [N*17] */
    double *s, *lam, *ds, *dlam, *rin; /* [N*mc]: 0..16 lower, 17..33 upper, 34.. corridor */
    double *corr;                       /* Mehrotra second-order term ds_aff*dlam_aff */
    int *nf;
    int twist;                          /* orc_options.twist */
    int tw_on;                          /* this iteration's Newton systems are solved the twisted way (see TW_EXACT_BELOW) */
} solver_ws;

static const double *face_A(const double *params, int M, int k) { return params + (size_t)k * (ORC_NPRE + 4 * M) + ORC_NPRE; }
static const double *face_b(const double *params, int M, int k) { return params + (size_t)k * (ORC_NPRE + 4 * M) + ORC_NPRE + 3 * M; }

/* G dz for constraint slot i of stage k */
static double gdz(const solver_ws *W, const double *params, int k, int i, const double *dzk)
{
    if (i < 17) return -dzk[i];
    if (i < 34) return dzk[i - 17];
    const double *a = face_A(params, W->M, k) + 3 * (i - 34);
    return a[0] * dzk[8] + a[1] * dzk[9] + a[2] * dzk[10];
}

/* assemble phi = grad f + G'(Sigma r_in + (sigma mu - corr)/s) for all stages */
static void build_phi(solver_ws *W, const double *params, double sigmamu, int use_corr)
{
    const int N = W->N, mc = W->mc;
    for (int k = 0; k < N; k++) {
        stage_ws *w = &W->st[k];
        const double *zk = W->z + 17 * k;
        double *phi = w->phi;
        for (int i = 0; i < 17; i++) phi[i] = w->hd[i] * zk[i] + w->q[i];
        for (int i = 0; i < 4; i++) {
            phi[i] += w->hc * zk[4 + i];
            phi[4 + i] += w->hc * zk[i];
        }
        const double *s = W->s + (size_t)k * mc, *l = W->lam + (size_t)k * mc, *r = W->rin + (size_t)k * mc;
        const double *cr = W->corr + (size_t)k * mc;
        for (int i = 0; i < 17; i++) {
            const double tl = (l[i] * r[i] + sigmamu - (use_corr ? cr[i] : 0.0)) / s[i];
            const double tu = (l[17 + i] * r[17 + i] + sigmamu - (use_corr ? cr[17 + i] : 0.0)) / s[17 + i];
            phi[i] += tu - tl;
        }
        const double *A = face_A(params, W->M, k);
        for (int j = 0; j < W->nf[k]; j++) {
            const int i = 34 + j;
            const double t = (l[i] * r[i] + sigmamu - (use_corr ? cr[i] : 0.0)) / s[i];
            phi[8] += A[3 * j] * t;
            phi[9] += A[3 * j + 1] * t;
            phi[10] += A[3 * j + 2] * t;
        }
    }
}

/* ------------------------------------------------------------------------------------------------------------------------
 * STUDY: the same Newton system solved from BOTH ends of the horizon.  Stages m..N-1 by the backward
 * recursion above, stages 0..m-1 by an ARRIVAL-cost recursion in information form,
 *     F_{k+1}(s+) = min_{w_k} [ l_k(u_k, w_k, x_k) + F_k(w_k, x_k) ],   u_k = w+ - d_w,   x_k = A^-1 (x+ - B u_k - d_x),
 * a 4x4 pivot on w_k and two 13x13 congruences per stage (the mirror image of a backward stage: u and w swap roles); the pinned
 * x_0 -- which makes the exact recursion rank-deficient for three stages -- enters as the penalty rho/2 |dx_0 - r_0|^2 (rho = 1e12:
 * tools/study/twisted_riccati.py).  The halves meet at stage m: ds_m = -(Q_m + P_m)^-1 (q_m + p_m); the first half is then
 * back-substituted m-1..0 and its multipliers are y_k = -(Q_k ds_k + q_k).  Switched on by the environment (ORC_TWIST=m, optional
 * ORC_TWIST_RHO): a study switch of the test oracle, never a product path.
 * ------------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    double Q[NS * NS], q[NS];          /* arrival cost AT s_k (before stage k's own cost)                         */
    double Lw[16], Hwr[4 * NS], G[NS * NS], Tt[NS * NS], tt[NS]; /* kept by the factorising pass for the vector pass */
    double Kw[4 * (NS + 1)];            /* w_k = -Kw [u; x; 1]                                                       */
} arr_ws;

static int chol(int n, const double *A, int lda, double *Lo) /* lower Cholesky, row-major n x n in Lo (ld n) */
{
    for (int j = 0; j < n; j++) {
        double dsum = A[j * lda + j];
        for (int l = 0; l < j; l++) dsum -= Lo[j * n + l] * Lo[j * n + l];
        if (!(dsum > 0.0)) return -1;
        const double dj = sqrt(dsum);
        Lo[j * n + j] = dj;
        for (int i = j + 1; i < n; i++) {
            double a = A[i * lda + j];
            for (int l = 0; l < j; l++) a -= Lo[i * n + l] * Lo[j * n + l];
            Lo[i * n + j] = a / dj;
        }
        for (int i = 0; i < j; i++) Lo[i * n + j] = 0.0;
    }
    return 0;
}
static void chol_solve(int n, const double *Lo, double *b) /* b <- (L L')^-1 b */
{
    for (int i = 0; i < n; i++) { double a = b[i]; for (int l = 0; l < i; l++) a -= Lo[i * n + l] * b[l]; b[i] = a / Lo[i * n + i]; }
    for (int i = n - 1; i >= 0; i--) { double a = b[i]; for (int l = i + 1; l < n; l++) a -= Lo[l * n + i] * b[l]; b[i] = a / Lo[i * n + i]; }
}
static int inv9(const double *A, double *Ai) /* Gauss-Jordan with partial pivoting */
{
    double M[9 * 18];
    for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) { M[i * 18 + j] = A[i * 9 + j]; M[i * 18 + 9 + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < 9; c++) {
        int piv = c;
        for (int i = c + 1; i < 9; i++) if (fabs(M[i * 18 + c]) > fabs(M[piv * 18 + c])) piv = i;
        if (M[piv * 18 + c] == 0.0) return -1;
        if (piv != c) for (int j = 0; j < 18; j++) { const double t = M[c * 18 + j]; M[c * 18 + j] = M[piv * 18 + j]; M[piv * 18 + j] = t; }
        const double inv = 1.0 / M[c * 18 + c];
        for (int j = 0; j < 18; j++) M[c * 18 + j] *= inv;
        for (int i = 0; i < 9; i++) if (i != c) { const double f = M[i * 18 + c]; if (f != 0.0) for (int j = 0; j < 18; j++) M[i * 18 + j] -= f * M[c * 18 + j]; }
    }
    for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) Ai[i * 9 + j] = M[i * 18 + 9 + j];
    return 0;
}
/* dense barrier-augmented Hessian of a stage over [u(0..3) w(4..7) x(8..16)], as riccati_step assembles it */
static void stage_phi_dense(const stage_ws *w, double *Q)
{
    memset(Q, 0, 17 * 17 * sizeof(double));
    for (int i = 0; i < 17; i++) Q[i * 17 + i] = w->PhiD[i];
    for (int i = 0; i < 4; i++) Q[i * 17 + 4 + i] = Q[(4 + i) * 17 + i] = w->hc;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Q[(8 + i) * 17 + 8 + j] += w->PhiPos[i * 3 + j];
    if (w->useH) {
        static const int zi[10] = {0, 1, 2, 3, 11, 12, 13, 14, 15, 16};
        for (int i = 0; i < 10; i++)
            for (int j = 0; j < 10; j++) Q[zi[i] * 17 + zi[j]] += w->thetaH * w->Hd[i * 10 + j];
    }
}
/* one arrival step: (a->Q, a->q) at s_k  ->  (Qn, qn) at s_{k+1}.  idx maps the 13 kept variables [u; x] to z positions. */
static int arrival_step(const stage_ws *w, arr_ws *a, double *Qn, double *qn, int full)
{
    static const int idx[NS] = {0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    double gf[17];
    memcpy(gf, w->phi, sizeof gf);
    for (int i = 0; i < NS; i++) gf[4 + i] += a->q[i];
    if (full) {
        double Hf[17 * 17];
        stage_phi_dense(w, Hf);
        for (int i = 0; i < NS; i++)
            for (int j = 0; j < NS; j++) Hf[(4 + i) * 17 + 4 + j] += a->Q[i * NS + j];
        double Hww[16];
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) Hww[i * 4 + j] = Hf[(4 + i) * 17 + 4 + j];
        if (chol(4, Hww, 4, a->Lw)) return -1;
        for (int i = 0; i < 4; i++) for (int j = 0; j < NS; j++) a->Hwr[i * NS + j] = Hf[(4 + i) * 17 + idx[j]];
        for (int j = 0; j < NS; j++) { /* Kw[:, j] = Hww^-1 Hwr[:, j] */
            double col[4];
            for (int i = 0; i < 4; i++) col[i] = a->Hwr[i * NS + j];
            chol_solve(4, a->Lw, col);
            for (int i = 0; i < 4; i++) a->Kw[i * (NS + 1) + j] = col[i];
        }
        for (int i = 0; i < NS; i++)
            for (int j = 0; j < NS; j++) {
                double v = Hf[idx[i] * 17 + idx[j]];
                for (int l = 0; l < 4; l++) v -= a->Hwr[l * NS + i] * a->Kw[l * (NS + 1) + j];
                a->G[i * NS + j] = v;
            }
        double Ai[81];
        if (inv9(w->Ax, Ai)) return -1;
        memset(a->Tt, 0, sizeof a->Tt);
        for (int i = 0; i < 4; i++) a->Tt[i * NS + i] = 1.0;
        for (int i = 0; i < 9; i++) {
            for (int j = 0; j < 4; j++) { double v = 0; for (int l = 0; l < 9; l++) v += Ai[i * 9 + l] * w->Bx[l * 4 + j]; a->Tt[(4 + i) * NS + j] = -v; }
            for (int j = 0; j < 9; j++) a->Tt[(4 + i) * NS + 4 + j] = Ai[i * 9 + j];
        }
        for (int i = 0; i < 4; i++) a->tt[i] = -w->d[i];
        for (int i = 0; i < 9; i++) {
            double v = 0;
            for (int l = 0; l < 9; l++) { double bd = -w->d[4 + l]; for (int j = 0; j < 4; j++) bd += w->Bx[l * 4 + j] * w->d[j]; v += Ai[i * 9 + l] * bd; }
            a->tt[4 + i] = v;
        }
        double GT[NS * NS];
        for (int i = 0; i < NS; i++) for (int j = 0; j < NS; j++) { double v = 0; for (int l = 0; l < NS; l++) v += a->G[i * NS + l] * a->Tt[l * NS + j]; GT[i * NS + j] = v; }
        for (int i = 0; i < NS; i++) for (int j = 0; j < NS; j++) { double v = 0; for (int l = 0; l < NS; l++) v += a->Tt[l * NS + i] * GT[l * NS + j]; Qn[i * NS + j] = v; }
        for (int i = 0; i < NS; i++) for (int j = 0; j < i; j++) { const double v = 0.5 * (Qn[i * NS + j] + Qn[j * NS + i]); Qn[i * NS + j] = Qn[j * NS + i] = v; }
    }
    /* vector part */
    double col[4], gg[NS], t2[NS];
    for (int i = 0; i < 4; i++) col[i] = gf[4 + i];
    chol_solve(4, a->Lw, col);
    for (int i = 0; i < 4; i++) a->Kw[i * (NS + 1) + NS] = col[i];
    for (int i = 0; i < NS; i++) { double v = gf[idx[i]]; for (int l = 0; l < 4; l++) v -= a->Hwr[l * NS + i] * col[l]; gg[i] = v; }
    for (int i = 0; i < NS; i++) { double v = gg[i]; for (int l = 0; l < NS; l++) v += a->G[i * NS + l] * a->tt[l]; t2[i] = v; }
    for (int i = 0; i < NS; i++) { double v = 0; for (int l = 0; l < NS; l++) v += a->Tt[l * NS + i] * t2[l]; qn[i] = v; }
    return 0;
}

static int kkt_solve_twisted(solver_ws *W, const double *xinit, int full, int m, double rho)
{
    const int N = W->N;
    static __thread arr_ws *A = 0;
    static __thread int A_n = 0;
    if (A_n < m + 1) { free(A); A = (arr_ws *)malloc(sizeof(arr_ws) * (size_t)(m + 1)); A_n = m + 1; }
    for (int k = N - 1; k >= m; k--) {
        const double *Pn = (k < N - 1) ? W->st[k + 1].P : 0, *pn = (k < N - 1) ? W->st[k + 1].p : 0;
        if (riccati_step(&W->st[k], Pn, pn, full)) return -1;
    }
    if (full) { memset(A[0].Q, 0, sizeof A[0].Q); for (int i = 0; i < 9; i++) A[0].Q[(4 + i) * NS + 4 + i] = rho; }
    memset(A[0].q, 0, sizeof A[0].q);
    for (int i = 0; i < 9; i++) A[0].q[4 + i] = -rho * (xinit[i] - W->z[8 + i]);
    for (int k = 0; k < m; k++)
        if (arrival_step(&W->st[k], &A[k], A[k + 1].Q, A[k + 1].q, full)) return -1;
    /* the halves meet at s_m */
    double S[NS * NS], Ls[NS * NS], ds[NS], dsn[NS];
    for (int i = 0; i < NS * NS; i++) S[i] = A[m].Q[i] + W->st[m].P[i];
    if (chol(NS, S, NS, Ls)) return -1;
    for (int i = 0; i < NS; i++) ds[i] = -(A[m].q[i] + W->st[m].p[i]);
    chol_solve(NS, Ls, ds);
    double dsm[NS];
    memcpy(dsm, ds, sizeof ds);
    /* second half forward (the loop of kkt_solve from stage m) */
    for (int k = m; k < N; k++) {
        const stage_ws *w = &W->st[k];
        double *dzk = W->dz + 17 * k, *yn = W->ynew + NS * k;
        for (int i = 0; i < NS; i++) { double a = w->p[i]; for (int j = 0; j < NS; j++) a += w->P[i * NS + j] * ds[j]; yn[i] = a; }
        double t[4], du[4];
        for (int i = 0; i < 4; i++) { double a = w->kt[i]; for (int j = 0; j < NS; j++) a += w->Kt[i * NS + j] * ds[j]; t[i] = -a; }
        for (int i = 3; i >= 0; i--) { double a = t[i]; for (int l = i + 1; l < 4; l++) a -= w->L[l * 4 + i] * du[l]; du[i] = a / w->L[i * 4 + i]; }
        for (int i = 0; i < 4; i++) dzk[i] = du[i];
        for (int i = 0; i < NS; i++) dzk[4 + i] = ds[i];
        if (k < N - 1) {
            for (int i = 0; i < 4; i++) dsn[i] = du[i] + w->d[i];
            for (int i = 0; i < 9; i++) {
                double a = w->d[4 + i];
                for (int j = 0; j < 9; j++) a += w->Ax[i * 9 + j] * ds[4 + j];
                for (int j = 0; j < 4; j++) a += w->Bx[i * 4 + j] * du[j];
                dsn[4 + i] = a;
            }
            memcpy(ds, dsn, sizeof ds);
        }
    }
    /* first half backward: [u; x]_k = Tt s_{k+1} + tt, w_k = -Kw [u; x; 1], y_k = -(Q_k ds_k + q_k) */
    double sp[NS];
    memcpy(sp, dsm, sizeof sp);
    for (int k = m - 1; k >= 0; k--) {
        const arr_ws *a = &A[k];
        double ux[NS], wk[4];
        for (int i = 0; i < NS; i++) { double v = a->tt[i]; for (int l = 0; l < NS; l++) v += a->Tt[i * NS + l] * sp[l]; ux[i] = v; }
        for (int i = 0; i < 4; i++) { double v = a->Kw[i * (NS + 1) + NS]; for (int l = 0; l < NS; l++) v += a->Kw[i * (NS + 1) + l] * ux[l]; wk[i] = -v; }
        double *dzk = W->dz + 17 * k, *yn = W->ynew + NS * k;
        for (int i = 0; i < 4; i++) { dzk[i] = ux[i]; dzk[4 + i] = wk[i]; }
        for (int i = 0; i < 9; i++) dzk[8 + i] = ux[4 + i];
        for (int i = 0; i < 4; i++) sp[i] = wk[i];
        for (int i = 0; i < 9; i++) sp[4 + i] = ux[4 + i];
        for (int i = 0; i < NS; i++) { double v = a->q[i]; for (int l = 0; l < NS; l++) v += a->Q[i * NS + l] * sp[l]; yn[i] = -v; }
    }
    return 0;
}

/* The twisted solve is an inexact Newton method: the penalty that pins x_0 leaves an equality residual ~ |y_0| / rho and a
 * direction error ~ 1e-5 relative.  Far from the solution that is immaterial; close to it the iteration would stall above tight
 * tolerances (measured on the hard family at 1e-8: 84 of 96 instances end in MAXIT).  So an iteration is solved the twisted way
 * only while the residuals of the PREVIOUS iteration (max of equality, inequality, stationarity, complementarity) exceed
 * TW_EXACT_BELOW = the reference's tolerance 1e-4 -- a solve at the default tolerances has converged by then and stays twisted
 * throughout, a solve at tighter tolerances finishes exactly; thresholds down to 1e-5 reach 1e-8 on every hard instance the plain
 * solve does, 1e-6 loses 4 of 1988 --; ALL iterations after that (one-way switch) are exact Newton steps of the plain recursion -- the end game, and
 * with it the accuracy of the returned point, is the plain solve's.  (The previous iteration's: the HIP kernel has to know before its model
 * phase, which writes the first-half records in another form.)  Same rule, same constant in csrc/frp_ipm_lds.hip. */
#define TW_EXACT_BELOW 1e-4

/* backward (full or vector-only) + forward sweep; fills W->dz and W->ynew */
static int kkt_solve(solver_ws *W, const double *xinit, int full)
{
    const int N = W->N;
    {
        static int tw_m = -2;
        static double tw_rho = 1e12;
        if (tw_m == -2) { const char *e = getenv("ORC_TWIST"); tw_m = e ? atoi(e) : -1; const char *r = getenv("ORC_TWIST_RHO"); if (r) tw_rho = atof(r); }
        const int m = tw_m > 0 ? tw_m : (W->twist < 0 ? 9 * N / 20 : W->twist);
        if (W->tw_on && m > 1 && m < N - 1 && N >= 4) return kkt_solve_twisted(W, xinit, full, m, tw_rho);
    }
    for (int k = N - 1; k >= 0; k--) {
        const double *Pn = (k < N - 1) ? W->st[k + 1].P : 0, *pn = (k < N - 1) ? W->st[k + 1].p : 0;
        if (riccati_step(&W->st[k], Pn, pn, full)) return -1;
    }
    /* stage 0: dx_0 = xinit - x_0, dw_0 from Pww dw = -(Pwx dx + p_w) */
    double ds[NS], dsn[NS];
    {
        const stage_ws *w = &W->st[0];
        for (int i = 0; i < 9; i++) ds[4 + i] = xinit[i] - W->z[8 + i];
        double Lw[16], rhs[4];
        memset(Lw, 0, sizeof Lw);
        for (int j = 0; j < 4; j++) {
            double dsum = w->P[j * NS + j];
            for (int l = 0; l < j; l++) dsum -= Lw[j * 4 + l] * Lw[j * 4 + l];
            if (!(dsum > 0.0)) return -1;
            Lw[j * 4 + j] = sqrt(dsum);
            for (int i = j + 1; i < 4; i++) {
                double a = w->P[i * NS + j];
                for (int l = 0; l < j; l++) a -= Lw[i * 4 + l] * Lw[j * 4 + l];
                Lw[i * 4 + j] = a / Lw[j * 4 + j];
            }
        }
        for (int i = 0; i < 4; i++) {
            double a = w->p[i];
            for (int j = 0; j < 9; j++) a += w->P[i * NS + 4 + j] * ds[4 + j];
            rhs[i] = -a;
        }
        for (int i = 0; i < 4; i++) {
            double a = rhs[i];
            for (int l = 0; l < i; l++) a -= Lw[i * 4 + l] * rhs[l];
            rhs[i] = a / Lw[i * 4 + i];
        }
        for (int i = 3; i >= 0; i--) {
            double a = rhs[i];
            for (int l = i + 1; l < 4; l++) a -= Lw[l * 4 + i] * rhs[l];
            rhs[i] = a / Lw[i * 4 + i];
        }
        for (int i = 0; i < 4; i++) ds[i] = rhs[i];
    }
    for (int k = 0; k < N; k++) {
        const stage_ws *w = &W->st[k];
        double *dzk = W->dz + 17 * k, *yn = W->ynew + NS * k;
        for (int i = 0; i < NS; i++) {
            double a = w->p[i];
            for (int j = 0; j < NS; j++) a += w->P[i * NS + j] * ds[j];
            yn[i] = a;
        }
        double t[4], du[4];
        for (int i = 0; i < 4; i++) {
            double a = w->kt[i];
            for (int j = 0; j < NS; j++) a += w->Kt[i * NS + j] * ds[j];
            t[i] = -a;
        }
        for (int i = 3; i >= 0; i--) {
            double a = t[i];
            for (int l = i + 1; l < 4; l++) a -= w->L[l * 4 + i] * du[l];
            du[i] = a / w->L[i * 4 + i];
        }
        for (int i = 0; i < 4; i++) dzk[i] = du[i];
        for (int i = 0; i < NS; i++) dzk[4 + i] = ds[i];
        if (k < N - 1) {
            for (int i = 0; i < 4; i++) dsn[i] = du[i] + w->d[i];
            for (int i = 0; i < 9; i++) {
                double a = w->d[4 + i];
                for (int j = 0; j < 9; j++) a += w->Ax[i * 9 + j] * ds[4 + j];
                for (int j = 0; j < 4; j++) a += w->Bx[i * 4 + j] * du[j];
                dsn[4 + i] = a;
            }
            memcpy(ds, dsn, sizeof ds);
        }
    }
    return 0;
}

#ifdef ORC_TRACE
static int trace_kp, trace_ip, trace_kd, trace_id;
#endif
/* ds, dlam from dz; returns max feasible step fractions (unscaled) through *ap, *ad */
static void slack_steps(solver_ws *W, const double *params, double sigmamu, int use_corr, double *ap, double *ad)
{
    const int N = W->N, mc = W->mc;
    double a_p = 1e300, a_d = 1e300;
    for (int k = 0; k < N; k++) {
        const double *dzk = W->dz + 17 * k;
        const int cnt = 34 + W->nf[k];
        for (int i = 0; i < cnt; i++) {
            const size_t id = (size_t)k * mc + i;
            const double dsi = -W->rin[id] - gdz(W, params, k, i, dzk);
            const double rc = W->s[id] * W->lam[id] - sigmamu + (use_corr ? W->corr[id] : 0.0);
            const double dli = (-rc - W->lam[id] * dsi) / W->s[id];
            W->ds[id] = dsi;
            W->dlam[id] = dli;
            if (dsi < 0.0) { const double a = -W->s[id] / dsi; if (a < a_p) { a_p = a;
#ifdef ORC_TRACE
                    trace_kp = k; trace_ip = i;
#endif
                } }
            if (dli < 0.0) { const double a = -W->lam[id] / dli; if (a < a_d) { a_d = a;
#ifdef ORC_TRACE
                    trace_kd = k; trace_id = i;
#endif
                } }
        }
    }
#ifdef ORC_TRACE
    if (use_corr) {
        const size_t ip = (size_t)trace_kp * mc + trace_ip, idd = (size_t)trace_kd * mc + trace_id;
        fprintf(stderr, "  primal blocked a=%.3g by stage %d row %d (s %.3g lam %.3g ds %.3g dl %.3g rin %.3g) | dual a=%.3g by stage %d row %d (s %.3g lam %.3g ds %.3g dl %.3g)\n",
                a_p, trace_kp, trace_ip, W->s[ip], W->lam[ip], W->ds[ip], W->dlam[ip], W->rin[ip],
                a_d, trace_kd, trace_id, W->s[idd], W->lam[idd], W->ds[idd], W->dlam[idd]);
    }
#endif
    *ap = a_p;
    *ad = a_d;
}

/* orc_solve_trace (test infrastructure): what iteration `k` of a solve factorises, recorded by orc_solve when set */
typedef struct {
    int k, done;
    double *z, *y, *theta, *H;
    int *exact;
} orc_trace;
static __thread orc_trace *tl_trace = 0;

int orc_solve(int N, int M, int model, const double *xinit, const double *z0,
              const double *params, const int *nfaces, const orc_options *opt_in,
              double *zout, orc_info *info)
{
    orc_options opt;
    if (opt_in) opt = *opt_in; else orc_default_options(&opt);
    const int np = ORC_NPRE + 4 * M, mc = 34 + M;
    solver_ws W;
    W.N = N; W.M = M; W.mc = mc;
    W.twist = opt_in ? opt_in->twist : 0;
    /* per-thread scratch, grown on demand and reused across solves (a calloc/free pair per solve
     * serialises 100+ OpenMP threads on the allocator) */
    static __thread stage_ws *tl_st = 0;
    static __thread double *tl_buf = 0;
    static __thread int *tl_nf = 0;
    static __thread size_t tl_nst = 0, tl_nbuf = 0;
    const size_t need_buf = (size_t)N * (17 * 2 + NS * 2 + 6 * mc);
    if (tl_nst < (size_t)N) {
        free(tl_st); free(tl_nf);
        tl_st = (stage_ws *)malloc((size_t)N * sizeof(stage_ws));
        tl_nf = (int *)malloc((size_t)N * sizeof(int));
        tl_nst = (size_t)N;
    }
    if (tl_nbuf < need_buf) {
        free(tl_buf);
        tl_buf = (double *)malloc(need_buf * sizeof(double));
        tl_nbuf = need_buf;
    }
    memset(tl_st, 0, (size_t)N * sizeof(stage_ws));
    memset(tl_buf, 0, need_buf * sizeof(double));
    memset(tl_nf, 0, (size_t)N * sizeof(int));
    W.st = tl_st;
    double *buf = tl_buf;
    W.z = buf; W.dz = W.z + 17 * N; W.y = W.dz + 17 * N; W.ynew = W.y + NS * N;
    W.s = W.ynew + NS * N; W.lam = W.s + (size_t)N * mc; W.ds = W.lam + (size_t)N * mc;
    W.dlam = W.ds + (size_t)N * mc; W.rin = W.dlam + (size_t)N * mc; W.corr = W.rin + (size_t)N * mc;
    W.nf = tl_nf;
    double lb[17], ub[17];
    orc_bounds(lb, ub);
    memcpy(W.z, z0, sizeof(double) * 17 * N);

    int mtot = 0;
    double smin = 1e300;
    for (int k = 0; k < N; k++) {
        const double *A = face_A(params, M, k), *b = face_b(params, M, k);
        int nf;
        if (nfaces) nf = nfaces[k];
        else { /* padded rows are all-zero rows at the tail (forces_normal.cpp:127-135) */
            nf = M;
            while (nf > 0 && A[3 * (nf - 1)] == 0.0 && A[3 * (nf - 1) + 1] == 0.0 && A[3 * (nf - 1) + 2] == 0.0 && b[nf - 1] >= -HU_OFF) nf--;
        }
        W.nf[k] = nf;
        mtot += 34 + nf;
        orc_cost_quadratic(params + (size_t)k * np, stage_class_of(k, N), model, W.st[k].hd, &W.st[k].hc, W.st[k].q, 0);
        const double *zk = W.z + 17 * k;
        double *s = W.s + (size_t)k * mc;
        for (int i = 0; i < 17; i++) {
            s[i] = zk[i] - lb[i];
            s[17 + i] = ub[i] - zk[i];
        }
        for (int j = 0; j < nf; j++)
            s[34 + j] = -(A[3 * j] * zk[8] + A[3 * j + 1] * zk[9] + A[3 * j + 2] * zk[10] - b[j] - HU_OFF);
        for (int i = 0; i < 34 + nf; i++) smin = fmin(smin, s[i]);
    }
    /* Infeasible-start initialisation: if the guess is not S_MIN-strictly inside all inequality
     * constraints, shift ALL slacks uniformly so that the smallest one is S_MIN + (worst violation);
     * the uniform slack residual is then removed by the (linear) Newton steps. */
    {
        const double shift = (smin >= S_MIN) ? 0.0 : (S_MIN - smin) + fmax(0.0, -smin);
        for (int k = 0; k < N; k++) {
            double *s = W.s + (size_t)k * mc, *l = W.lam + (size_t)k * mc;
            for (int i = 0; i < 34 + W.nf[k]; i++) {
                s[i] += shift;
                l[i] = opt.mu0 / s[i];
            }
        }
    }

    int flag = ORC_MAXIT, it = 0, nfallback = 0;
    /* weight of the dynamics Hessian: 1 = exact Hessian.  An indefinite Riccati pivot block redoes the iteration with
     * the Gauss-Newton Hessian, quarters the weight, and it recovers by 0.1 per successful iteration (alternating
     * between the two Hessians at full weight can cycle for 100+ iterations on a locally non-convex problem). */
    double theta_h = 1.0;
    orc_info inf;
    memset(&inf, 0, sizeof inf);
    W.tw_on = 1;
    for (it = 0;; it++) {
        /* ---- evaluate model, residuals ---- */
        double res_eq = 0, res_in = 0, rs = 0, rcomp = 0, gap = 0, pobj = 0;
        for (int i = 0; i < 9; i++) res_eq = fmax(res_eq, fabs(xinit[i] - W.z[8 + i]));
        for (int k = 0; k < N; k++) {
            stage_ws *w = &W.st[k];
            const double *zk = W.z + 17 * k, *pk = params + (size_t)k * np;
            if (k < N - 1) {
                double xn[9];
                const double *zn = zk + 17;
                orc_rk2(zk + 8, zk, pk + 3, xn, w->Ax, w->Bx);
                for (int i = 0; i < 4; i++) w->d[i] = zk[i] - zn[4 + i];
                for (int i = 0; i < 9; i++) w->d[4 + i] = xn[i] - zn[8 + i];
                for (int i = 0; i < NS; i++) res_eq = fmax(res_eq, fabs(w->d[i]));
            }
            /* inequality residuals r = G z - g + s */
            double *s = W.s + (size_t)k * mc, *l = W.lam + (size_t)k * mc, *r = W.rin + (size_t)k * mc;
            for (int i = 0; i < 17; i++) {
                r[i] = lb[i] - zk[i] + s[i];
                r[17 + i] = zk[i] - ub[i] + s[17 + i];
                res_in = fmax(res_in, fmax(lb[i] - zk[i], zk[i] - ub[i]));
            }
            const double *A = face_A(params, M, k), *b = face_b(params, M, k);
            for (int j = 0; j < W.nf[k]; j++) {
                const double hj = A[3 * j] * zk[8] + A[3 * j + 1] * zk[9] + A[3 * j + 2] * zk[10] - b[j] - HU_OFF;
                r[34 + j] = hj + s[34 + j];
                res_in = fmax(res_in, hj);
            }
            for (int i = 0; i < 34 + W.nf[k]; i++) {
                res_in = fmax(res_in, fabs(r[i]));
                rcomp = fmax(rcomp, s[i] * l[i]);
                gap += s[i] * l[i];
            }
            /* stationarity: grad f + M' y_{k+1} - [0; y_k] + G' lam */
            double g[17], fk;
            for (int i = 0; i < 17; i++) g[i] = w->hd[i] * zk[i] + w->q[i];
            for (int i = 0; i < 4; i++) { g[i] += w->hc * zk[4 + i]; g[4 + i] += w->hc * zk[i]; }
            orc_stage_eval(zk, pk, M, stage_class_of(k, N), model, &fk, 0, 0, 0, 0, 0);
            pobj += fk;
            for (int i = 0; i < 17; i++) g[i] += l[17 + i] - l[i];
            for (int j = 0; j < W.nf[k]; j++)
                for (int c = 0; c < 3; c++) g[8 + c] += A[3 * j + c] * l[34 + j];
            const double *yk = W.y + NS * k;
            for (int i = 0; i < NS; i++) g[4 + i] -= yk[i];
            if (k < N - 1) {
                const double *yn = W.y + NS * (k + 1);
                for (int j = 0; j < 4; j++) {
                    double a = yn[j];
                    for (int i = 0; i < 9; i++) a += w->Bx[i * 4 + j] * yn[4 + i];
                    g[j] += a;
                }
                for (int j = 0; j < 9; j++) {
                    double a = 0;
                    for (int i = 0; i < 9; i++) a += w->Ax[i * 9 + j] * yn[4 + i];
                    g[8 + j] += a;
                }
            }
            for (int i = 0; i < 17; i++) rs = fmax(rs, fabs(g[i]));
        }
        const double mu = gap / mtot;
        static double tw_below = -1.0; /* (ORC_TW_EXACT_BELOW in the environment: study knob) */
        if (tw_below < 0.0) { const char *e = getenv("ORC_TW_EXACT_BELOW"); tw_below = e ? atof(e) : TW_EXACT_BELOW; }
        const int tw_next = fmax(fmax(res_eq, res_in), fmax(rs, rcomp)) > tw_below; /* (for the NEXT iteration: see TW_EXACT_BELOW) */
        inf.it = it; inf.res_eq = res_eq; inf.res_ineq = res_in; inf.rsnorm = rs; inf.rcompnorm = rcomp;
        inf.pobj = pobj; inf.mu = mu;
        if (!(res_eq == res_eq) || !(rs == rs) || !(pobj == pobj)) { flag = ORC_BADFUNCEVAL; break; }
        if (res_eq <= opt.tol_eq && res_in <= opt.tol_ineq && rs <= opt.tol_stat && rcomp <= opt.tol_comp) { flag = ORC_OPTIMAL; break; }
        if (it >= opt.maxit) { flag = ORC_MAXIT; break; }
        /* divergence guard = early exit of (locally) infeasible instances: without a feasible point the multipliers, and with
         * them the average complementarity mu, grow geometrically while the primal residuals stagnate.  Measured on 12 k
         * converging problems of the BASELINE workloads mu never exceeds 5 after the first iteration (one outlier), whereas
         * the infeasible instances of configs[3] cross 10 at iteration 15 on average (and 1e6 at 30).  The default of the
         * option is a conservative 1e3 (a hard but feasible problem must not be declared hopeless on a margin of 1.4 x);
         * 10 is what the configs[3] benchmark opts into. */
        if (mu > (opt.diverge_mu > 0.0 ? opt.diverge_mu : 1e3) * fmax(1.0, opt.mu0) || rs > DIVERGE_RS) { flag = ORC_NOPROGRESS; break; }

        /* ---- barrier-augmented Hessian ---- */
        for (int k = 0; k < N; k++) {
            stage_ws *w = &W.st[k];
            const double *s = W.s + (size_t)k * mc, *l = W.lam + (size_t)k * mc;
            for (int i = 0; i < 17; i++) w->PhiD[i] = w->hd[i] + l[i] / s[i] + l[17 + i] / s[17 + i];
            memset(w->PhiPos, 0, sizeof w->PhiPos);
            const double *A = face_A(params, M, k);
            for (int j = 0; j < W.nf[k]; j++) {
                const double sg = l[34 + j] / s[34 + j];
                for (int a = 0; a < 3; a++)
                    for (int c = 0; c < 3; c++) w->PhiPos[a * 3 + c] += sg * A[3 * j + a] * A[3 * j + c];
            }
        }
        /* ---- exact Lagrangian Hessian of the dynamics (optional), Gauss-Newton fallback ---- */
        const int want_exact = (opt.hessian == 1) || (opt.hessian == 2 && res_eq <= EXACT_SWITCH_EQ);
        for (int k = 0; k < N; k++) {
            stage_ws *w = &W.st[k];
            w->useH = 0;
            if (want_exact && k < N - 1) {
                const double *zk = W.z + 17 * k, *yn = W.y + NS * (k + 1);
                orc_rk2_hess(zk + 8, zk, params + (size_t)k * np + 3, yn + 4, yn + 7, w->Hd);
                w->useH = 1;
                w->thetaH = theta_h;
            }
        }
        /* ---- predictor ---- */
        double ap, ad;
        build_phi(&W, params, 0.0, 0);
        int frc = kkt_solve(&W, xinit, 1);
        if (frc && want_exact) { /* indefinite reduced Hessian: redo with the Gauss-Newton Hessian */
            for (int k = 0; k < N; k++) W.st[k].useH = 0;
            frc = kkt_solve(&W, xinit, 1);
            nfallback++;
            theta_h *= THETA_DOWN;
        } else if (want_exact) {
            theta_h = fmin(1.0, theta_h + THETA_UP);
        }
        if (tl_trace && it == tl_trace->k) { /* the iterate, y, and each stage's Hessian as the predictor factorised it (no barrier terms) */
            orc_trace *t = tl_trace;
            memcpy(t->z, W.z, sizeof(double) * 17 * N);
            memcpy(t->y, W.y, sizeof(double) * NS * N);
            *t->exact = N > 1 && W.st[0].useH;
            *t->theta = N > 1 ? W.st[0].thetaH : 1.0;
            for (int k = 0; k < N; k++) {
                stage_ws bare = W.st[k];
                for (int i = 0; i < 17; i++) bare.PhiD[i] = bare.hd[i];
                memset(bare.PhiPos, 0, sizeof bare.PhiPos);
                stage_phi_dense(&bare, t->H + (size_t)k * 289);
            }
            t->done = 1;
        }
        if (frc) { flag = ORC_FACTORIZATION_ERROR; break; }
        slack_steps(&W, params, 0.0, 0, &ap, &ad);
        ap = fmin(1.0, ap); ad = fmin(1.0, ad);
        double gap_aff = 0;
        for (int k = 0; k < N; k++)
            for (int i = 0; i < 34 + W.nf[k]; i++) {
                const size_t id = (size_t)k * mc + i;
                gap_aff += (W.s[id] + ap * W.ds[id]) * (W.lam[id] + ad * W.dlam[id]);
                W.corr[id] = W.ds[id] * W.dlam[id];
            }
        const double mu_aff = gap_aff / mtot;
        double sigma = mu_aff / mu;
        sigma = sigma * sigma * sigma;
        if (sigma > 1.0) sigma = 1.0;
        inf.mu_aff = mu_aff; inf.sigma = sigma; inf.step_aff = ap;
        /* centring target, floored so that complementarity is not driven (far) below its tolerance
         * while stationarity / feasibility are still converging (Gauss-Newton: linear rate) */
        double smu = sigma * mu;
        if (smu < MU_FLOOR_FRAC * opt.tol_comp) smu = MU_FLOOR_FRAC * opt.tol_comp;
        /* ---- corrector ---- */
        build_phi(&W, params, smu, 1);
        if (kkt_solve(&W, xinit, 0)) { flag = ORC_FACTORIZATION_ERROR; break; }
        slack_steps(&W, params, smu, 1, &ap, &ad);
        ap = fmin(1.0, opt.ftb * ap); ad = fmin(1.0, opt.ftb * ad);
        inf.step_cc = ap;
        for (int k = 0; k < N; k++) {
            for (int i = 0; i < 17; i++) W.z[17 * k + i] += ap * W.dz[17 * k + i];
            for (int i = 0; i < NS; i++) W.y[NS * k + i] += ap * (W.ynew[NS * k + i] - W.y[NS * k + i]);
            for (int i = 0; i < 34 + W.nf[k]; i++) {
                const size_t id = (size_t)k * mc + i;
                W.s[id] += ap * W.ds[id];
                W.lam[id] += ad * W.dlam[id];
            }
        }
        /* multiplier safeguard (cf. Waechter & Biegler 2006, eq. 16, with a tight kappa): no complementarity
         * pair may fall below 1/KAPPA_LAM of the average one.  Pairs far below the central path have a
         * barrier weight lam/s that is too small for the Newton direction to "see" the constraint, and the
         * next steps get cut to a few percent by the fraction-to-boundary rule (jamming). */
        {
            double g2 = 0;
            for (int k = 0; k < N; k++)
                for (int i = 0; i < 34 + W.nf[k]; i++) { const size_t id = (size_t)k * mc + i; g2 += W.s[id] * W.lam[id]; }
            const double floor_prod = g2 / mtot / KAPPA_LAM;
            for (int k = 0; k < N; k++)
                for (int i = 0; i < 34 + W.nf[k]; i++) {
                    const size_t id = (size_t)k * mc + i;
                    if (W.lam[id] * W.s[id] < floor_prod) W.lam[id] = floor_prod / W.s[id];
                }
        }
        W.tw_on = W.tw_on && tw_next; /* (one way: an ill-conditioned instance whose residuals rise again stays on exact steps) */
    }
    memcpy(zout, W.z, sizeof(double) * 17 * N);
    inf.nfallback = nfallback;
    if (info) *info = inf;
    return flag;
}

void orc_solve_batch(int B, int N, int M, int model, const double *xinit, const double *z0,
                     const double *params, const int *nfaces, const orc_options *opt,
                     double *z, int *exitflag, orc_info *info, int nthreads)
{
    const size_t np = (size_t)N * (ORC_NPRE + 4 * M);
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#pragma omp parallel for schedule(dynamic, 1)
    for (int b = 0; b < B; b++) {
        orc_info inf;
        const int fl = orc_solve(N, M, model, xinit + 9 * (size_t)b, z0 + 17 * (size_t)N * b, params + np * b,
                                 nfaces ? nfaces + (size_t)N * b : 0, opt, z + 17 * (size_t)N * b, &inf);
        if (exitflag) exitflag[b] = fl;
        if (info) info[b] = inf;
    }
}

int orc_solve_trace(int N, int M, int model, const double *xinit, const double *z0, const double *params, const int *nfaces,
                    const orc_options *opt, int k, double *z, double *y, double *theta, int *exact, double *H)
{
    orc_options o;
    if (opt) o = *opt; else orc_default_options(&o);
    if (o.maxit > k + 1) o.maxit = k + 1; /* (nothing after iteration k is recorded) */
    orc_trace t = {k, 0, z, y, theta, H, exact};
    double *zo = (double *)malloc(sizeof(double) * 17 * (size_t)N);
    tl_trace = &t;
    orc_solve(N, M, model, xinit, z0, params, nfaces, &o, zo, 0);
    tl_trace = 0;
    free(zo);
    return t.done;
}
