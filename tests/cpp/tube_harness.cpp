// Test harness: the tube kernel's per-lane arithmetic (forces_resilient_planner_amd/csrc/frp_tube_math.hpp, the very text the
// gfx950 kernel compiles) run on the CPU, one planner after the other, so that the CPU suite can compare it with the
// multiprecision fixture.  What the kernel does across lanes -- adding the three channels of a stage, the Minkowski recursion
// over the stages, the position block -- is restated here in the kernel's order of operations (frp_tube.hip: tube_kernel).
//   tube_harness <in.bin> <out.bin>
//   in : int32 C, then per case: int32 N, int32 force_panels (0 = the kernel's own choice), double consts[9] = mass drag ego_r
//        ego_h noise[3] epsilon Ts, double plan[N][17]
//   out: per case, per stage: double E[9], Qd[45], G[27], nu, panels   (83 doubles; panels = 0 marks a stage outside the domain)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../forces_resilient_planner_amd/csrc/frp_tube_math.hpp"

using namespace frp;

static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: tube_harness in.bin out.bin\n"); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    int C; rd(&C, sizeof C, fi);
    for (int cs = 0; cs < C; ++cs) {
        int N, force; double c[9];
        rd(&N, sizeof N, fi); rd(&force, sizeof force, fi); rd(c, sizeof c, fi);
        if (N < 1 || N > 64) { fprintf(stderr, "bad horizon\n"); return 2; }
        std::vector<double> z((size_t)N * TB_NZ);
        rd(z.data(), z.size() * sizeof(double), fi);
        const double mass = c[0], drag = c[1], ego_r = c[2], ego_h = c[3], *noise = c + 4, epsilon = c[7], t = c[8];
        std::vector<double> Qd((size_t)N * TB_SYM), G((size_t)N * 27), Q1((size_t)N * 6), Q2((size_t)N * 6), trQd(N), nu(N), pan(N);
        for (int k = 0; k < N; ++k) {
            PhiS P; double R[9];
            build_phi(&z[(size_t)k * TB_NZ], mass, drag, P, R);
            int e = 0;
            for (int a = 0; a < 3; ++a)
                for (int cc = a; cc < 3; ++cc)
                    Q1[6 * k + e++] = ego_r * ego_r * (R[3 * a] * R[3 * cc] + R[3 * a + 1] * R[3 * cc + 1]) + ego_h * ego_h * R[3 * a + 2] * R[3 * cc + 2];
            nu[k] = phi_norm1(P) * t;
            int panels = tube_panels(nu[k]);
            pan[k] = panels;
            if (panels == 0) panels = TB_MAX_PANELS;
            if (force > 0) panels = force;
            double X[3][TB_SYM], rootTr[3];
            for (int ch = 0; ch < 3; ++ch) {
                for (int q = 0; q < TB_SYM; ++q) X[ch][q] = 0.0;
                tube_lane(P, t, panels, ch, &G[27 * k + 9 * ch], X[ch]);
                const double scale = t * noise[ch] * noise[ch];
                double tr = 0.0;
                for (int m = 0; m < 9; ++m) tr += X[ch][sym_index(m, m)];
                rootTr[ch] = sqrt(scale * tr);
                const double nrm = scale / rootTr[ch];
                for (int q = 0; q < TB_SYM; ++q) X[ch][q] *= nrm;
            }
            const double temp = rootTr[0] + rootTr[1] + rootTr[2];
            for (int q = 0; q < TB_SYM; ++q) Qd[(size_t)k * TB_SYM + q] = temp * (X[0][q] + X[1][q] + X[2][q]);
            trQd[k] = temp * temp;
        }
        // the stage recursion of Q_origin and the position block of exp(Phi t) Q exp(Phi' t)
        double qo[TB_SYM], trQo = 9.0 * epsilon * epsilon;
        for (int m = 0; m < 9; ++m)
            for (int n = m; n < 9; ++n) qo[sym_index(m, n)] = m == n ? epsilon * epsilon : 0.0;
        for (int s = 0; s < N; ++s) {
            const double beta = sqrt(trQo / trQd[s]), ca = 1.0 + 1.0 / beta, cb = 1.0 + beta;
            for (int q = 0; q < TB_SYM; ++q) qo[q] = ca * qo[q] + cb * Qd[(size_t)s * TB_SYM + q];
            trQo = ca * trQo + cb * trQd[s];
            const double *g = &G[27 * s];
            int e = 0;
            for (int a = 0; a < 3; ++a)
                for (int cc = a; cc < 3; ++cc) {
                    double acc = 0.0;
                    for (int m = 0; m < 9; ++m) {
                        double row = 0.0;
                        for (int n = 0; n < 9; ++n) row += qo[m <= n ? sym_index(m, n) : sym_index(n, m)] * g[9 * cc + n];
                        acc += g[9 * a + m] * row;
                    }
                    Q2[6 * s + e++] = acc;
                }
        }
        for (int k = 0; k < N; ++k) {
            double q[6], E[9];
            for (int e = 0; e < 6; ++e) q[e] = Q1[6 * k + e];
            if (k > 0) {
                const double *q2 = &Q2[6 * (k - 1)];
                const double beta = sqrt((q[0] + q[3] + q[5]) / (q2[0] + q2[3] + q2[5]));
                for (int e = 0; e < 6; ++e) q[e] = (1.0 + 1.0 / beta) * q[e] + (1.0 + beta) * q2[e];
            }
            sqrt_sym3(q, E);
            fwrite(E, sizeof(double), 9, fo);
            fwrite(&Qd[(size_t)k * TB_SYM], sizeof(double), TB_SYM, fo);
            fwrite(&G[27 * k], sizeof(double), 27, fo);
            fwrite(&nu[k], sizeof(double), 1, fo);
            fwrite(&pan[k], sizeof(double), 1, fo);
        }
    }
    fclose(fi); fclose(fo);
    return 0;
}
