// frp_capi.hip -- the C-ABI of libfrp_nmpc_amd.so (declared in include/frp_nmpc.h): version, options and the batched device-pointer
// API used by bench.py, the tests and the host-side adapter mirror.  Its other two parts are units of their own: the FORCES drop-in call
// (frp_dropin.hip) and the host-buffer batch calls (frp_host_batch.hip); frp_capi_internal.hpp declares what this unit defines for them.
// There is NO CPU compute path in these files: without a HIP device every entry point fails.
#include <cmath>
#include <cstring>
#include <mutex>
#include "frp_capi_internal.hpp"

static_assert(sizeof(frp_forces_params) == 23600, "params layout must match FORCESNLPsolver_normal.h:153-168");
static_assert(offsetof(frp_forces_params, x0) == 72, "x0 offset");
static_assert(offsetof(frp_forces_params, all_parameters) == 2792, "all_parameters offset");
static_assert(offsetof(frp_forces_params, num_of_threads) == 23592, "num_of_threads offset");
static_assert(sizeof(frp_forces_output) == 2720, "output layout must match FORCESNLPsolver_normal.h:173-236");
static_assert(sizeof(frp_forces_info) == 136, "info layout must match FORCESNLPsolver_normal.h:241-301");
static_assert(offsetof(frp_forces_info, res_eq) == 8 && offsetof(frp_forces_info, lsit_aff) == 96 &&
              offsetof(frp_forces_info, step_aff) == 104 && offsetof(frp_forces_info, fevalstime) == 128, "info offsets");

namespace {

// device allocation that is released on every exit path of the *_host helpers
struct DevMem {
    void *p = nullptr;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// Rate of the current device's wall clock (s_memrealtime) in Hz, cached per device; 0 when it cannot be queried.
double wall_clock_hz()
{
    static std::mutex m;
    static double hz[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) { (void)hipGetLastError(); return 0.0; }
    std::lock_guard<std::mutex> l(m);
    if (dev < 64 && hz[dev] > 0.0) return hz[dev];
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) { (void)hipGetLastError(); return 0.0; }
    const double r = 1e3 * (double)khz;
    if (dev < 64) hz[dev] = r;
    return r;
}

} // namespace

namespace frp::capi {

bool budget_args(double timeout, frp::KernelArgs *a)
{
    a->deadline = 0; a->origin = nullptr; a->timeout_invalid = 0;
    if (timeout == 0.0 || timeout == HUGE_VAL) return true;   // no budget
    if (!(timeout > 0.0)) { a->timeout_invalid = 1; return true; } // negative or NaN
    const double hz = wall_clock_hz();
    if (hz <= 0.0) return false;
    const double ticks = timeout * hz;
    if (ticks < 1.0) { a->timeout_invalid = 1; return true; }  // shorter than one tick of the clock
    if (ticks >= 4.6e18) return true;                          // (beyond 2^62 ticks -- centuries: no budget)
    a->deadline = (unsigned long long)std::ceil(ticks);
    return true;
}

bool batch_shape_ok(const frp_nmpc_batch *b)
{
    if (!b || b->B <= 0 || b->N < 2 || b->N > 64 || b->M < 0 || b->MF < 0 || b->MF > b->M || b->MF > frp::FRP_MAX_FACES) return false;
    if (!b->xinit || !b->x0 || !b->params || !b->z || !b->exitflag || !b->iters) return false;
    return b->model == FRP_MODEL_NORMAL || b->model == FRP_MODEL_FINAL;
}

bool fill_args(const frp_nmpc_batch *b, const frp_nmpc_options *opt_in, void *ws, size_t ws_bytes, frp::KernelArgs *a)
{
    if (!batch_shape_ok(b) || !ws || ws_bytes < frp::ws_bytes(b->B, b->N, b->MF)) return false;
    frp_nmpc_options o;
    if (opt_in) o = *opt_in; else frp_nmpc_default_options(&o);
    a->B = b->B; a->N = b->N; a->M = b->M; a->MF = b->MF; a->model = b->model; a->maxit = o.maxit;
    a->tol_stat = o.tol_stat; a->tol_eq = o.tol_eq; a->tol_ineq = o.tol_ineq; a->tol_comp = o.tol_comp;
    a->mu0 = o.mu0; a->ftb = o.ftb; a->hessian = o.hessian; a->twist = o.twist;
    a->diverge_mu = o.diverge_mu > 0.0 ? o.diverge_mu : 1e3;
    a->xinit = b->xinit; a->x0 = b->x0; a->params = b->params; a->nfaces = b->nfaces;
    a->z = b->z; a->exitflag = b->exitflag; a->iters = b->iters; a->info = b->info;
    a->ws = static_cast<double *>(ws);
    a->models = b->model_per_problem;
    a->order_hint = b->order_hint;
    a->counter = nullptr; a->order = nullptr;
    a->self_reset = 0;
    a->variant_B = 0;
    a->slot_reserve = 0;
    a->done_flag = nullptr; a->done_seq = 0;
    return budget_args(o.timeout, a);
}

} // namespace frp::capi

using frp::capi::fill_args;

extern "C" {

int frp_nmpc_abi_version(void) { return FRP_NMPC_ABI_VERSION; }

int frp_nmpc_abi_check(int abi_version, size_t options_bytes, size_t batch_bytes, int info_stride)
{
    if (abi_version == FRP_NMPC_ABI_VERSION && options_bytes == sizeof(frp_nmpc_options) && batch_bytes == sizeof(frp_nmpc_batch) && info_stride == FRP_INFO_STRIDE)
        return FRP_OK;
    fprintf(stderr, "[frp_nmpc] the caller was built against another frp_nmpc.h: ABI version %d (library %d), frp_nmpc_options %zu B (%zu), "
                    "frp_nmpc_batch %zu B (%zu), info stride %d (%d)\n",
            abi_version, FRP_NMPC_ABI_VERSION, options_bytes, sizeof(frp_nmpc_options), batch_bytes, sizeof(frp_nmpc_batch), info_stride, FRP_INFO_STRIDE);
    return FRP_ERR_ARG;
}

const char *frp_nmpc_version(void) { return "frp_nmpc_amd 0.6 (gfx950, FP64 interior point: three / four wavefronts per problem, stage records in LDS)"; }

int frp_nmpc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void frp_nmpc_default_options(frp_nmpc_options *o)
{
    o->maxit = 200;
    o->tol_stat = 1e-4;
    o->tol_eq = 1e-4;
    o->tol_ineq = 1e-4;
    o->tol_comp = 1e-4;
    o->mu0 = 1.0;
    o->ftb = 0.99;
    o->hessian = 1;
    o->diverge_mu = 1e3;
    o->twist = 0;
    o->timeout = 0.0;
}

size_t frp_nmpc_workspace_bytes(int B, int N, int MF) { return frp::ws_bytes(B, N, MF); }

int frp_nmpc_solve_batch(const frp_nmpc_batch *batch, const frp_nmpc_options *opt, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    frp::KernelArgs a;
    if (!fill_args(batch, opt, workspace, workspace_bytes, &a)) return FRP_ERR_ARG;
    FRP_HIP(frp::launch_ipm(a, static_cast<hipStream_t>(stream)));
    return FRP_OK;
}

int frp_nmpc_time_solve(const frp_nmpc_batch *batch, const frp_nmpc_options *opt, void *workspace,
                        size_t workspace_bytes, void *stream, int reps, float *avg_ms)
{
    frp::KernelArgs a;
    if (!fill_args(batch, opt, workspace, workspace_bytes, &a) || reps <= 0 || !avg_ms) return FRP_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    struct Events { // destroyed on every exit path
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    FRP_HIP(hipEventCreate(&ev.e0));
    FRP_HIP(hipEventCreate(&ev.e1));
    FRP_HIP(hipEventRecord(ev.e0, st));
    for (int r = 0; r < reps; r++) FRP_HIP(frp::launch_ipm(a, st));
    FRP_HIP(hipEventRecord(ev.e1, st));
    FRP_HIP(hipEventSynchronize(ev.e1));
    float ms = 0.f;
    FRP_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *avg_ms = ms / reps;
    return FRP_OK;
}

int frp_nmpc_kernel_timing_begin(int max_launches, int stride)
{
    if (max_launches <= 0 || stride <= 0) return FRP_ERR_ARG;
    return frp::kernel_timing_begin(max_launches, stride) == hipSuccess ? FRP_OK : FRP_ERR_ARG;
}

int frp_nmpc_kernel_timing_end(float *avg_ms, int *launches)
{
    if (!avg_ms || !launches) return FRP_ERR_ARG;
    const hipError_t rc = frp::kernel_timing_end(avg_ms, launches);
    return rc == hipSuccess ? FRP_OK : (rc == hipErrorInvalidValue ? FRP_ERR_ARG : FRP_ERR_HIP);
}

int frp_nmpc_set_q4_min_batch(int min_batch) { return frp::lds_q4_set_min_batch(min_batch); }

int frp_nmpc_solver_variant(const frp_nmpc_batch *batch, const frp_nmpc_options *opt, char *buf, size_t n)
{
    static double no_ws; // (the selection looks at the shape of the launch, never at the workspace)
    frp::KernelArgs a;
    frp_nmpc_options o; // (nor at the wall-clock budget)
    if (opt) o = *opt; else frp_nmpc_default_options(&o);
    o.timeout = 0.0;
    if (!buf || n == 0 || !fill_args(batch, &o, &no_ws, SIZE_MAX, &a)) return FRP_ERR_ARG;
    buf[0] = 0;
    if (frp_nmpc_device_count() <= 0) return FRP_ERR_NO_DEVICE; // (the choice depends on the device's CU count)
    const char *name = frp::ipm_variant_name(a);
    if (!name) return FRP_ERR_ARG;
    if (strlen(name) >= n) return FRP_ERR_ARG;
    memcpy(buf, name, strlen(name) + 1);
    return FRP_OK;
}

int frp_nmpc_stage_eval(int B, int N, int M, int model, const double *z, const double *params, double *f,
                        double *grad_f, double *c, double *jac_c, double *h, void *stream)
{
    if (B <= 0 || N < 2 || M < 0 || !z || !params) return FRP_ERR_ARG;
    FRP_HIP(frp::launch_stage_eval(B, N, M, model, z, params, f, grad_f, c, jac_c, h, static_cast<hipStream_t>(stream)));
    return FRP_OK;
}

int frp_nmpc_stage_eval_host(int B, int N, int M, int model, const double *z, const double *params, double *f,
                             double *grad_f, double *c, double *jac_c, double *h)
{
    if (B <= 0 || N < 2 || M < 0 || !z || !params) return FRP_ERR_ARG;
    if (frp_nmpc_device_count() <= 0) return FRP_ERR_NO_DEVICE;
    const size_t T = (size_t)B * N, np = FRP_NPAR(M);
    DevMem dz, dp, df, dg, dc, dJ, dh;
    FRP_HIP(dz.alloc(T * 17 * sizeof(double)));
    FRP_HIP(dp.alloc(T * np * sizeof(double)));
    FRP_HIP(hipMemcpy(dz.p, z, T * 17 * sizeof(double), hipMemcpyHostToDevice));
    FRP_HIP(hipMemcpy(dp.p, params, T * np * sizeof(double), hipMemcpyHostToDevice));
    if (f) FRP_HIP(df.alloc(T * sizeof(double)));
    if (grad_f) FRP_HIP(dg.alloc(T * 17 * sizeof(double)));
    if (c) FRP_HIP(dc.alloc(T * 13 * sizeof(double)));
    if (jac_c) FRP_HIP(dJ.alloc(T * 221 * sizeof(double)));
    if (h && M > 0) FRP_HIP(dh.alloc(T * M * sizeof(double)));
    const int rc = frp_nmpc_stage_eval(B, N, M, model, dz.as<double>(), dp.as<double>(), df.as<double>(), dg.as<double>(),
                                       dc.as<double>(), dJ.as<double>(), dh.as<double>(), nullptr);
    if (rc != FRP_OK) return rc;
    FRP_HIP(hipDeviceSynchronize());
    if (f) FRP_HIP(hipMemcpy(f, df.p, T * sizeof(double), hipMemcpyDeviceToHost));
    if (grad_f) FRP_HIP(hipMemcpy(grad_f, dg.p, T * 17 * sizeof(double), hipMemcpyDeviceToHost));
    if (c) FRP_HIP(hipMemcpy(c, dc.p, T * 13 * sizeof(double), hipMemcpyDeviceToHost));
    if (jac_c) FRP_HIP(hipMemcpy(jac_c, dJ.p, T * 221 * sizeof(double), hipMemcpyDeviceToHost));
    if (dh.p) FRP_HIP(hipMemcpy(h, dh.p, T * M * sizeof(double), hipMemcpyDeviceToHost));
    return FRP_OK;
}

} // extern "C"
