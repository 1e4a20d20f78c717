// frp_dropin.hip -- the FORCES drop-in call of libfrp_nmpc_amd.so: FORCESNLPsolver_normal_solve / FORCESNLPsolver_final_solve with the
// reference's struct layouts (FORCESNLPsolver_normal.h:153-301,317-323; asserted in frp_capi.hip), so plan_manage's adapters
// (forces_normal.cpp:139, forces_final.cpp:138) link against this library unchanged.  No CPU compute path: without a HIP device the call fails.
#include <chrono>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <mutex>
#include "frp_capi_internal.hpp"
#include "frp_model.hpp"

namespace {
using frp::capi::fill_args;

// ---- single-problem context of the drop-in ABI: created lazily on first call, freed at unload
// (the reference has no init/teardown call; SURVEY 8b "Ownership"). Serialised by a mutex: the
// reference library is not re-entrant either (static work arrays).
// The inputs are staged in ONE pinned, device-mapped block and the outputs land in another:
//   in  (doubles): xinit(9) | x0(340) | all_parameters(2600) | nfaces(20 ints)
//   out (doubles): z(340) | info(FRP_INFO_STRIDE) | exitflag, iterations (2 ints)
// With at most 15 live corridor rows per stage (the kernel variants that read every input ONCE, at the start of the solve) the kernel
// reads and writes those blocks in place over PCIe -- no copy commands around the launch, and no reset launch in front of it
// (KernelArgs::self_reset): one call = one kernel launch and one stream synchronisation.  More rows (the variants that re-read
// the rows every iteration) or FRP_NMPC_DROPIN_ZEROCOPY=0: one host-to-device and one device-to-host copy through the same blocks.
//   out (doubles): plan(340) | info(FRP_INFO_STRIDE) | (exitflag, iterations) | (completion word, pad)
// In-place calls do not synchronise the stream either: the kernel stores the call's sequence number into the completion word (system-scope
// release, behind a fence and a barrier over all its outputs) and the caller spins on it -- the runtime's own completion path costs ~10 us
// of a 130 us call.
constexpr int DI_IN_DOUBLES = 9 + 340 + 2600 + 10, DI_OUT_DOUBLES = 340 + FRP_INFO_STRIDE + 2;
struct DropInCtx {
    bool ready = false;
    hipStream_t stream = nullptr;
    double *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr, *d_ws = nullptr;
    double *m_in = nullptr, *m_out = nullptr; // device addresses of the pinned blocks (null: not mapped, copies only)
    int seq = 0;                              // completion word of the last in-place call
    size_t ws_bytes = 0;
    frp_forces_extfunc probed[2] = {nullptr, nullptr}; // the callback last probed per model (a different pointer is probed again)
    bool probe_ok[2] = {false, false};
    std::mutex mtx;
    ~DropInCtx();
};
DropInCtx g_ctx;
void ctx_release();
DropInCtx::~DropInCtx() { if (ready) ctx_release(); }

void ctx_release()
{
    if (g_ctx.d_in) (void)hipFree(g_ctx.d_in);
    if (g_ctx.d_out) (void)hipFree(g_ctx.d_out);
    if (g_ctx.d_ws) (void)hipFree(g_ctx.d_ws);
    if (g_ctx.h_in) (void)hipHostFree(g_ctx.h_in);
    if (g_ctx.h_out) (void)hipHostFree(g_ctx.h_out);
    if (g_ctx.stream) (void)hipStreamDestroy(g_ctx.stream);
    g_ctx.d_in = g_ctx.d_out = g_ctx.d_ws = g_ctx.h_in = g_ctx.h_out = g_ctx.m_in = g_ctx.m_out = nullptr;
    g_ctx.stream = nullptr;
    g_ctx.ready = false;
}

int ctx_init()
{
    if (g_ctx.ready) return FRP_OK;
    if (frp_nmpc_device_count() <= 0) return FRP_ERR_NO_DEVICE;
    g_ctx.ws_bytes = std::max(frp::ws_bytes(1, FRP_N_REF, FRP_NH_REF), frp::ws_bytes(1, FRP_N_REF, 6)); // (the size depends on the face count: every shape a call can have)
    // (a failure half way leaves nothing behind: the next call starts from scratch)
    const bool ok = hipStreamCreate(&g_ctx.stream) == hipSuccess &&
                    hipMalloc(&g_ctx.d_in, DI_IN_DOUBLES * sizeof(double)) == hipSuccess &&
                    hipMalloc(&g_ctx.d_out, DI_OUT_DOUBLES * sizeof(double)) == hipSuccess &&
                    hipHostMalloc(&g_ctx.h_in, DI_IN_DOUBLES * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
                    hipHostMalloc(&g_ctx.h_out, DI_OUT_DOUBLES * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
                    hipMalloc(&g_ctx.d_ws, g_ctx.ws_bytes) == hipSuccess &&
                    hipMemset(g_ctx.d_ws, 0, 64) == hipSuccess; // (the queue head: zero between calls, see KernelArgs::self_reset)
    if (!ok) {
        fprintf(stderr, "[frp_nmpc] HIP error %s while creating the drop-in context\n", hipGetErrorString(hipGetLastError()));
        ctx_release();
        return FRP_ERR_HIP;
    }
    const char *zc = getenv("FRP_NMPC_DROPIN_ZEROCOPY");
    if (!(zc && atoi(zc) == 0)) {
        void *pi = nullptr, *po = nullptr;
        if (hipHostGetDevicePointer(&pi, g_ctx.h_in, 0) == hipSuccess && hipHostGetDevicePointer(&po, g_ctx.h_out, 0) == hipSuccess) {
            g_ctx.m_in = static_cast<double *>(pi); g_ctx.m_out = static_cast<double *>(po);
        } else {
            (void)hipGetLastError();
        }
    }
    std::memset(g_ctx.h_out, 0, DI_OUT_DOUBLES * sizeof(double)); g_ctx.seq = 0; // (the completion word starts at 0; sequence numbers at 1)
    g_ctx.ready = true;
    return FRP_OK;
}

// Probe a caller-supplied model callback against the built-in device model at fixed test points
// (all three stage classes).  The callback is never used for the solve itself.
bool probe_callback(frp_forces_extfunc fn, int model)
{
    const int stages[3] = {0, 7, 19};
    for (int s = 0; s < 3; s++) {
        double z[17] = {0.1, -0.05, 0.2, 7.5, 0.02, 0.01, -0.03, 7.3, 0.5, -0.3, 1.2, 0.4, 0.1, -0.2, 0.05, -0.1, 0.3};
        double p[130];
        std::memset(p, 0, sizeof p);
        const double p10[10] = {1, 0, 1, 0.5, -1, 0.2, 15, 3, 80, 0.2};
        std::memcpy(p, p10, sizeof p10);
        p[10] = 1.0; p[11] = 0.5; p[12] = -0.25; p[100] = 2.0;
        double y[13] = {0}, lam[64] = {0}, f = 0, g[17] = {0}, c[13] = {0}, J[221] = {0}, h[30] = {0}, Jh[510] = {0};
        fn(z, y, lam, p, &f, g, c, J, h, Jh, nullptr, stages[s], 0, 0);
        const int sc = frp::stage_class(stages[s], FRP_N_REF);
        double g2[17];
        const double f2 = frp::stage_cost(z, p, sc, model, g2);
        if (std::fabs(f - f2) > 1e-9 * (1.0 + std::fabs(f2))) return false;
        for (int i = 0; i < 17; i++)
            if (std::fabs(g[i] - g2[i]) > 1e-9 * (1.0 + std::fabs(g2[i]))) return false;
        if (sc != frp::STAGE_LAST) {
            frp::Lin L;
            double xn[9];
            frp::rk2<true>(z + 8, z, p + 3, xn, &L);
            for (int i = 0; i < 9; i++)
                if (std::fabs(c[i] - xn[i]) > 1e-9 * (1.0 + std::fabs(xn[i]))) return false;
            const double *Lc = reinterpret_cast<const double *>(&L);
            for (int i = 0; i < 9; i++) {
                for (int j = 0; j < 4; j++)
                    if (std::fabs(J[j * 13 + i] - frp::lin_B(Lc, i, j)) > 1e-9) return false;
                for (int j = 0; j < 9; j++)
                    if (std::fabs(J[(8 + j) * 13 + i] - frp::lin_A(Lc, i, j)) > 1e-9) return false;
            }
        }
        const double h0 = 1.0 * z[8] + 0.5 * z[9] - 0.25 * z[10] - 2.0;
        if (std::fabs(h[0] - h0) > 1e-9) return false;
    }
    return true;
}

int forces_solve(int model, frp_forces_params *params, frp_forces_output *output, frp_forces_info *info, FILE *fs,
                 frp_forces_extfunc fn)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!params || !output || !info) return FRP_EXIT_PARAM_VALUE;
    std::lock_guard<std::mutex> lock(g_ctx.mtx);
    std::memset(info, 0, sizeof *info);
    if (const int rc = ctx_init(); rc != FRP_OK) {
        // not a parameter error: "solver not valid on this machine" (the reference's -100) or a failed runtime call (-101)
        if (fs) fprintf(fs, rc == FRP_ERR_NO_DEVICE ? "frp_nmpc: no usable HIP device -- this library has no CPU path\n"
                                                      : "frp_nmpc: the HIP runtime failed while creating the solver context\n");
        return rc == FRP_ERR_NO_DEVICE ? FRP_EXIT_NO_DEVICE : FRP_EXIT_DEVICE_FAULT;
    }
    if (fn) {
        if (g_ctx.probed[model] != fn) {
            g_ctx.probe_ok[model] = probe_callback(fn, model);
            g_ctx.probed[model] = fn;
        }
        if (!g_ctx.probe_ok[model]) {
            if (fs) fprintf(fs, "frp_nmpc: the supplied model callback differs from the built-in device model\n");
            return FRP_EXIT_PARAM_VALUE;
        }
    }
    for (int i = 0; i < 9; i++) if (!std::isfinite(params->xinit[i])) return FRP_EXIT_PARAM_VALUE;
    hipStream_t st = g_ctx.stream;
    // stage the inputs; count the live corridor rows here (600 rows): trailing all-zero rows are the padding
    // forces_normal.cpp:127-135 writes -- with the counts the kernel variant that keeps the rows in registers runs
    double *hin = g_ctx.h_in;
    std::memcpy(hin, params->xinit, 9 * sizeof(double));
    std::memcpy(hin + 9, params->x0, 340 * sizeof(double));
    std::memcpy(hin + 349, params->all_parameters, 2600 * sizeof(double));
    int *hnf = reinterpret_cast<int *>(hin + 2949);
    int mf = 0;
    for (int k = 0; k < FRP_N_REF; k++) {
        const double *pk = params->all_parameters + (size_t)k * FRP_NPAR(FRP_NH_REF);
        int nf = FRP_NH_REF;
        while (nf > 0) {
            const double *r = pk + FRP_NPRE + 3 * (nf - 1);
            if (r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0 && pk[FRP_NPRE + 3 * FRP_NH_REF + nf - 1] >= -frp::HU) nf--;
            else break;
        }
        hnf[k] = nf;
        mf = nf > mf ? nf : mf;
    }
    auto device_fault = [&](const char *what) { // a runtime failure is not the caller's parameters: its own code, the context rebuilt on the next call
        fprintf(stderr, "[frp_nmpc] HIP error %s in the drop-in solve (%s)\n", hipGetErrorString(hipGetLastError()), what);
        if (fs) fprintf(fs, "frp_nmpc: HIP runtime failure during the solve (%s)\n", what);
        (void)hipStreamSynchronize(st);
        ctx_release();
        return FRP_EXIT_DEVICE_FAULT;
    };
    // in place over PCIe when the kernel variant reads its inputs once (mf <= 15: the corridor rows live in registers)
    const bool zero_copy = g_ctx.m_in && g_ctx.m_out && mf <= 15;
    double *din = zero_copy ? g_ctx.m_in : g_ctx.d_in, *dout = zero_copy ? g_ctx.m_out : g_ctx.d_out;
    if (!zero_copy && hipMemcpyAsync(g_ctx.d_in, hin, DI_IN_DOUBLES * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return device_fault("copy in");
    frp_nmpc_batch b;
    std::memset(&b, 0, sizeof b);
    b.B = 1; b.N = FRP_N_REF; b.M = FRP_NH_REF; b.MF = mf; b.model = model;
    b.xinit = din; b.x0 = din + 9; b.params = din + 349; b.nfaces = reinterpret_cast<const int *>(din + 2949);
    b.z = dout; b.info = dout + 340;
    b.exitflag = reinterpret_cast<int *>(dout + 340 + FRP_INFO_STRIDE); b.iters = b.exitflag + 1;
    frp::KernelArgs a;
    // FORCES' entry point has no options argument: the one option a caller of a SINGLE solve may want -- the latency option
    // frp_nmpc_options.twist -- comes from the environment (FRP_NMPC_TWIST = m or -1; unset / 0: the plain solve)
    static const int env_twist = [] { const char *e = getenv("FRP_NMPC_TWIST"); return e ? atoi(e) : 0; }();
    // ... and so does the wall-clock budget of one call, frp_nmpc_options.timeout (FRP_NMPC_TIMEOUT = seconds; unset: none)
    static const double env_timeout = [] { const char *e = getenv("FRP_NMPC_TIMEOUT"); return e && *e ? strtod(e, nullptr) : 0.0; }();
    frp_nmpc_options opt;
    frp_nmpc_default_options(&opt);
    opt.twist = env_twist;
    opt.timeout = env_timeout;
    if (!fill_args(&b, &opt, g_ctx.d_ws, g_ctx.ws_bytes, &a)) return FRP_EXIT_PARAM_VALUE;
    if (a.timeout_invalid) { // nothing is solved: the initial guess comes back (FORCESNLPsolver_normal.h:136)
        std::memcpy(output->x, params->x0, 340 * sizeof(double));
        if (fs) fprintf(fs, "INVALID_TIMEOUT - the wall-clock budget FRP_NMPC_TIMEOUT is negative, NaN or shorter than one clock tick\n");
        return FRP_EXIT_INVALID_TIMEOUT;
    }
    a.self_reset = 1;
    int *h_done = reinterpret_cast<int *>(g_ctx.h_out + 340 + FRP_INFO_STRIDE + 1);
    if (zero_copy) {
        g_ctx.seq = g_ctx.seq == 0x7fffffff ? 1 : g_ctx.seq + 1;
        a.done_flag = reinterpret_cast<int *>(g_ctx.m_out + 340 + FRP_INFO_STRIDE + 1); a.done_seq = g_ctx.seq;
    }
    if (frp::launch_ipm(a, st) != hipSuccess) return device_fault("launch");
    bool seen = false;
    if (zero_copy) { // (a solve is ~0.1 ms; the caller's thread spins for at most 2 ms -- twenty ordinary solves -- then blocks in the runtime's own wait like the call it replaces: a MAXIT solve or a device fault does not burn a real-time thread for the whole tick)
        const auto t_spin = std::chrono::steady_clock::now();
        for (unsigned n = 0;; n++) {
            if (__atomic_load_n(h_done, __ATOMIC_ACQUIRE) == g_ctx.seq) { seen = true; break; }
            if ((n & 1023u) == 1023u && std::chrono::steady_clock::now() - t_spin > std::chrono::milliseconds(2)) break;
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#elif defined(__aarch64__)
            asm volatile("yield" ::: "memory");
#endif
        }
    }
    if (!seen &&
        ((!zero_copy && hipMemcpyAsync(g_ctx.h_out, g_ctx.d_out, DI_OUT_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) ||
         hipStreamSynchronize(st) != hipSuccess))
        return device_fault("copy out / synchronise");
    std::memcpy(output->x, g_ctx.h_out, 340 * sizeof(double));
    const double *inf = g_ctx.h_out + 340;
    const int *fi = reinterpret_cast<const int *>(g_ctx.h_out + 340 + FRP_INFO_STRIDE);
    const int flag = fi[0], it = fi[1];
    info->it = it; info->it2opt = it;
    info->res_eq = inf[0]; info->res_ineq = inf[1]; info->rsnorm = inf[2]; info->rcompnorm = inf[3];
    info->pobj = inf[4]; info->mu = inf[5]; info->step_cc = inf[6];
    // affine-step quantities of the last iteration taken (FORCESNLPsolver_normal.h:275-289); no line search exists, so the two
    // backtracking counters stay 0
    info->mu_aff = inf[8]; info->sigma = inf[9]; info->step_aff = inf[10];
    // duality gap of the local QP model at the returned point = sum of slack * multiplier over all inequalities (what an
    // interior-point method drives to zero; mu is its mean); dobj = pobj - dgap (:262-270)
    info->dgap = inf[11]; info->dobj = inf[4] - inf[11];
    info->rdgap = std::fabs(inf[11]) / std::fmax(std::fabs(inf[4]), 1e-300);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    info->solvetime = secs;
    info->fevalstime = 0.0; /* model evaluation is fused into the device kernel */
    if (fs) {
        if (flag == FRP_EXIT_OPTIMAL)
            fprintf(fs, "OPTIMAL (within EQTOL=%.1e, INEQTOL=%.1e, STATTOL=%.1e, COMPTOL=%.1e)\n", a.tol_eq, a.tol_ineq, a.tol_stat, a.tol_comp);
        else if (flag == FRP_EXIT_MAXIT)
            fprintf(fs, "MAXIT - Maximum number of iterations reached, exiting.\n");
        else
            fprintf(fs, "exit flag %d\n", flag);
        fprintf(fs, "Solve time: %5.3f ms (%d iterations)\n", secs * 1e3, it);
    }
    return flag;
}

} // namespace

extern "C" {

int FORCESNLPsolver_normal_solve(frp_forces_params *params, frp_forces_output *output, frp_forces_info *info,
                                 FILE *fs, frp_forces_extfunc evalextfunctions)
{
    return forces_solve(FRP_MODEL_NORMAL, params, output, info, fs, evalextfunctions);
}

int FORCESNLPsolver_final_solve(frp_forces_params *params, frp_forces_output *output, frp_forces_info *info,
                                FILE *fs, frp_forces_extfunc evalextfunctions)
{
    return forces_solve(FRP_MODEL_FINAL, params, output, info, fs, evalextfunctions);
}

} // extern "C"
