// frp_host_batch.hip -- the host-buffer batch calls of libfrp_nmpc_amd.so (declared in include/frp_nmpc.h): frp_nmpc_solve_batch_host,
// the registry of pinned caller buffers (frp_nmpc_host_register ...) and the pipelined pair frp_nmpc_solve_batch_host_begin / _wait.
// Host-buffer batch: persistent device buffers and pinned staging (grown on demand, freed at unload), the batch cut into chunks
// whose copies and solves overlap on three streams: chunk c + 1 is staged and copied in while chunk c solves and chunk c - 1
// copies out.  Serialised by a mutex (one pipeline per process).
#include <cstring>
#include <algorithm>
#include <mutex>
#include <vector>
#include "frp_capi_internal.hpp"
#include "frp_copy_pool.hpp"

namespace {
using namespace frp::capi;

// One chunk of nb problems of the caller's batch h on the device.  Input block, in doubles:
//   xinit | x0 | params (Md live rows of the caller's M) | nfaces | models   (the int arrays padded to (N + 1) / 2 and 1 double per problem)
// output block of a staged chunk:  z | info | exitflag | iterations (ints).  gather_inputs_kernel below writes the same input block.
// With explicit face counts only the first MF corridor rows of a stage can be live (a larger count is a parameter error the
// kernel reports either way): the staging copy packs the parameters to MF rows -- 26.4 -> 8.9 KB per problem over PCIe at
// the reference's 30-row layout with 6-face corridors -- and the device solves the same problems in the compact layout.
struct ChunkLayout {
    bool has_nf, has_md;
    int M, Md;                                    // corridor rows of the caller's layout / of the device-side one (Md < M: packed)
    size_t nb, N, np_h, np;                       // problems, stages, parameter doubles per stage in the two layouts
    size_t x0, params, nfaces, models, in_bytes;  // offsets in doubles; bytes of the whole input block
    size_t info, flags, out_bytes;
    ChunkLayout(const frp_nmpc_batch *h, size_t nb_)
        : has_nf(h->nfaces), has_md(h->model_per_problem), M(h->M), Md(has_nf && h->MF < M ? h->MF : M), nb(nb_), N((size_t)h->N), np_h(FRP_NPAR(M)), np(FRP_NPAR(Md))
    {
        x0 = nb * 9; params = x0 + nb * N * 17; nfaces = params + nb * N * np;
        models = nfaces + (has_nf ? nb * ((N + 1) / 2) : 0);
        in_bytes = (models + (has_md ? nb : 0)) * sizeof(double);
        info = nb * N * 17; flags = info + (h->info ? nb * FRP_INFO_STRIDE : 0);
        out_bytes = (flags + nb) * sizeof(double);
    }
    // the input pointers of the device-side batch whose block starts at `base`
    void point_inputs(frp_nmpc_batch *d, const double *base) const
    {
        d->B = (int)nb; d->M = Md;
        d->xinit = base; d->x0 = base + x0; d->params = base + params;
        d->nfaces = has_nf ? reinterpret_cast<const int *>(base + nfaces) : nullptr;
        d->model_per_problem = has_md ? reinterpret_cast<const int *>(base + models) : nullptr;
    }
};

struct HostPipe {
    std::mutex mtx;
    bool ready = false;
    int device = -1;    // the device the streams, events and buffers below belong to (the one current at their creation)
    hipStream_t s_in = nullptr, s_solve = nullptr, s_out = nullptr;
    unsigned long long *d_origin = nullptr; // origin of the wall-clock budget of a call: shared by all its chunks (KernelArgs::origin)
    static constexpr int NSLOT = 3;
    struct Slot {
        double *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr, *d_ws = nullptr;
        size_t in_bytes = 0, out_bytes = 0, ws_bytes = 0;
        hipEvent_t e_in = nullptr, e_solve = nullptr, e_out = nullptr;
    } slot[NSLOT];
    // The pipeline (streams, events, device and pinned buffers) belongs to ONE device: the one current when it was built.  A call
    // made with another device current rebuilds it there (the per-call allocation it replaced worked on any device).
    int ensure(int dev)
    {
        if (ready && device != dev) {
            const int prev = device;
            (void)hipSetDevice(prev);
            drain_all();
            release();
            FRP_HIP(hipSetDevice(dev));
        }
        if (ready) return FRP_OK;
        device = dev;
        ready = true; // (from here on release() owns whatever was created; a failure half way releases it again)
        bool ok = hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithFlags(&s_solve, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void **>(&d_origin), 64) == hipSuccess;
        for (auto &s : slot)
            ok = ok && hipEventCreateWithFlags(&s.e_in, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&s.e_solve, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&s.e_out, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            fprintf(stderr, "[frp_nmpc] HIP error %s while creating the host-batch pipeline\n", hipGetErrorString(hipGetLastError()));
            release();
            return FRP_ERR_HIP;
        }
        return FRP_OK;
    }
    void release()
    {
        if (!ready) return;
        for (auto &s : slot) {
            (void)hipFree(s.d_in); (void)hipFree(s.d_out); (void)hipFree(s.d_ws); (void)hipHostFree(s.h_in); (void)hipHostFree(s.h_out);
            if (s.e_in) (void)hipEventDestroy(s.e_in);
            if (s.e_solve) (void)hipEventDestroy(s.e_solve);
            if (s.e_out) (void)hipEventDestroy(s.e_out);
            s = Slot();
        }
        if (s_in) (void)hipStreamDestroy(s_in);
        if (s_solve) (void)hipStreamDestroy(s_solve);
        if (s_out) (void)hipStreamDestroy(s_out);
        if (d_origin) (void)hipFree(d_origin);
        s_in = s_solve = s_out = nullptr; d_origin = nullptr;
        ready = false; device = -1;
    }
    void drain_all()
    {
        if (s_in) (void)hipStreamSynchronize(s_in);
        if (s_solve) (void)hipStreamSynchronize(s_solve);
        if (s_out) (void)hipStreamSynchronize(s_out);
    }
    ~HostPipe() { release(); }
};
HostPipe g_pipe;

// ---- caller buffers registered with frp_nmpc_host_register: pinned in place and mapped into the device's address space.  A batch whose
// arrays ALL lie in registered ranges needs no staging: a gather kernel reads the live part of a chunk's inputs straight from the
// caller's memory over PCIe into the chunk's device block (what the staging copy + hipMemcpyAsync did, without the host's memcpy, which
// set the pace: 16 host threads against a 0.85 ms solve), and the solver writes plans, flags and diagnostics in place.
struct HostRegistry {
    // refs: registrations of exactly this base (a second registration of the same pointer is counted, the pages are unpinned by the
    // last unregistration).  A registration that lies INSIDE a range somebody else registered is kept as an alias of that range
    // (nothing is pinned for it; it is unregistered by its own pointer like any other; the owner cannot leave while it has aliases).
    struct Range { char *base; size_t bytes; char *dev; int refs; };
    struct Alias { char *ptr; char *owner; };
    std::mutex mtx;
    std::vector<Range> ranges;
    std::vector<Alias> aliases;
    Range *containing(const char *c, size_t bytes)
    {
        for (Range &r : ranges)
            if (c >= r.base && c + bytes <= r.base + r.bytes) return &r;
        return nullptr;
    }
    template <typename T>
    T *device_ptr(const T *p, size_t bytes)
    {
        const char *c = reinterpret_cast<const char *>(p);
        const Range *r = p ? containing(c, bytes) : nullptr;
        return r ? reinterpret_cast<T *>(r->dev + (c - r->base)) : nullptr;
    }
    // m = the batch h with its nine arrays at their device addresses; true when every array h has lies inside ranges the caller registered:
    // no staging (the caller holds mtx)
    bool resolve(const frp_nmpc_batch *h, frp_nmpc_batch *m)
    {
        const size_t Bz = (size_t)h->B, Tz = Bz * (size_t)h->N;
        *m = *h;
        m->xinit = device_ptr(h->xinit, Bz * 9 * 8); m->x0 = device_ptr(h->x0, Tz * 17 * 8); m->params = device_ptr(h->params, Tz * FRP_NPAR(h->M) * 8);
        m->nfaces = device_ptr(h->nfaces, Tz * 4); m->model_per_problem = device_ptr(h->model_per_problem, Bz * 4);
        m->z = device_ptr(h->z, Tz * 17 * 8); m->info = device_ptr(h->info, Bz * FRP_INFO_STRIDE * 8);
        m->exitflag = device_ptr(h->exitflag, Bz * 4); m->iters = device_ptr(h->iters, Bz * 4);
        return m->xinit && m->x0 && m->params && (!h->nfaces || m->nfaces) && (!h->model_per_problem || m->model_per_problem) && m->z && (!h->info || m->info) && m->exitflag && m->iters;
    }
};
HostRegistry g_reg;

// ---- two batches in flight (frp_nmpc_solve_batch_host_begin / _wait; registered buffers only): while batch k solves, the gather kernel of
// batch k + 1 reads its inputs over the host link.  The solver's workgroups are persistent and fill every CU's registers, so a gather block
// that arrives later finds no room until a solver workgroup retires: the pipelined solves leave `reserve` resident slots free (KernelArgs::
// slot_reserve) and the gather runs as a SMALL persistent grid of that many workgroups (64 suffice for the link: tools/ubench/zc_read).
struct AsyncPipe {
    static constexpr int GATHER_WGS = 64;
    std::mutex mtx;
    bool ready = false;
    int device = -1;
    hipStream_t s_gather = nullptr, s_solve = nullptr;
    static constexpr int NSLOT = 2;
    struct Slot {
        double *d_in = nullptr, *d_ws = nullptr;
        size_t in_bytes = 0, ws_bytes = 0;
        hipEvent_t e_in = nullptr, e_done = nullptr;
        bool busy = false;
    } slot[NSLOT];
    int ensure(int dev)
    {
        if (ready && device != dev) { // (the pipeline belongs to the device it was built on; a call from another one rebuilds it there)
            const int prev = device;
            (void)hipSetDevice(prev);
            release();
            FRP_HIP(hipSetDevice(dev));
        }
        if (ready) return FRP_OK;
        device = dev; ready = true;
        bool ok = hipStreamCreateWithFlags(&s_gather, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithFlags(&s_solve, hipStreamNonBlocking) == hipSuccess;
        for (auto &s : slot)
            ok = ok && hipEventCreateWithFlags(&s.e_in, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&s.e_done, hipEventDisableTiming) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); release(); return FRP_ERR_HIP; }
        return FRP_OK;
    }
    void release()
    {
        for (auto &s : slot) {
            if (s.busy && s.e_done) (void)hipEventSynchronize(s.e_done);
            (void)hipFree(s.d_in); (void)hipFree(s.d_ws);
            if (s.e_in) (void)hipEventDestroy(s.e_in);
            if (s.e_done) (void)hipEventDestroy(s.e_done);
            s = Slot();
        }
        if (s_gather) (void)hipStreamDestroy(s_gather);
        if (s_solve) (void)hipStreamDestroy(s_solve);
        s_gather = s_solve = nullptr; ready = false; device = -1;
    }
    ~AsyncPipe() { release(); }
};
AsyncPipe g_async;

// one chunk's device block [xinit | x0 | params (Md live rows of the caller's M) | nfaces | models] from the caller's (mapped) arrays
__global__ __launch_bounds__(256) void gather_inputs_kernel(size_t nb, size_t N, int M, int Md, const double *__restrict__ xinit, const double *__restrict__ x0,
                                                            const double *__restrict__ params, const int *__restrict__ nfaces, const int *__restrict__ models,
                                                            double *__restrict__ d_in)
{
    const size_t np_h = FRP_NPAR(M), np = FRP_NPAR(Md), n_x = nb * 9, n_z = nb * N * 17, n_p = nb * N * np, nf_d = nfaces ? (N + 1) / 2 : 0;
    const size_t total = n_x + n_z + n_p, stride = (size_t)gridDim.x * blockDim.x;
    const size_t head = 10 + 3 * (size_t)Md, boff = 10 + 3 * (size_t)M;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        double v;
        if (i < n_x) v = xinit[i];
        else if (i < n_x + n_z) v = x0[i - n_x];
        else {
            const size_t q = i - n_x - n_z, row = q / np, e = q - row * np;
            v = params[row * np_h + (e < head ? e : e - head + boff)];
        }
        d_in[i] = v;
    }
    int *d_nf = reinterpret_cast<int *>(d_in + total);
    if (nfaces)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb * N; i += stride) d_nf[i] = nfaces[i];
    if (models) {
        int *d_md = reinterpret_cast<int *>(d_in + total + nb * nf_d);
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += stride) d_md[i] = models[i];
    }
}

// the gather of the chunk L that starts at problem b0 of the resolved batch m, into the block d_in
void launch_gather(const ChunkLayout &L, const frp_nmpc_batch &m, size_t b0, unsigned blocks, double *d_in, hipStream_t st)
{
    hipLaunchKernelGGL(gather_inputs_kernel, dim3(blocks), dim3(256), 0, st, L.nb, L.N, L.M, L.Md, m.xinit + b0 * 9, m.x0 + b0 * L.N * 17,
                       m.params + b0 * L.N * L.np_h, m.nfaces ? m.nfaces + b0 * L.N : nullptr, m.model_per_problem ? m.model_per_problem + b0 : nullptr, d_in);
}

// a slot's buffer grows to the largest request it has seen: device memory and, where the slot stages, the pinned block of the same size
int grow(double *&dev, double **pinned, size_t &have, size_t want)
{
    if (want <= have) return FRP_OK;
    (void)hipFree(dev); dev = nullptr; have = 0;
    if (pinned) { (void)hipHostFree(*pinned); *pinned = nullptr; }
    FRP_HIP(hipMalloc(&dev, want));
    if (pinned) FRP_HIP(hipHostMalloc(pinned, want, hipHostMallocDefault));
    have = want;
    return FRP_OK;
}
} // namespace

extern "C" {

int frp_nmpc_host_register(void *ptr, size_t bytes)
{
    if (!ptr || !bytes) return FRP_ERR_ARG;
    if (frp_nmpc_device_count() <= 0) return FRP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lock(g_reg.mtx);
    char *c = reinterpret_cast<char *>(ptr);
    if (HostRegistry::Range *r = g_reg.containing(c, bytes)) {
        if (r->base == c) r->refs++;                    // the same buffer once more: counted
        else g_reg.aliases.push_back({c, r->base});     // inside somebody's range: an alias, unregistered by its own pointer
        return FRP_OK;
    }
    // a range that OVERLAPS a registered one without lying inside it cannot be pinned a second time by the runtime: refuse it by name
    for (const HostRegistry::Range &r : g_reg.ranges)
        if (c < r.base + r.bytes && r.base < c + bytes) return FRP_ERR_ARG;
    if (hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); return FRP_ERR_HIP; }
    void *dev = nullptr;
    if (hipHostGetDevicePointer(&dev, ptr, 0) != hipSuccess || !dev) { (void)hipHostUnregister(ptr); (void)hipGetLastError(); return FRP_ERR_HIP; }
    g_reg.ranges.push_back({c, bytes, reinterpret_cast<char *>(dev), 1});
    return FRP_OK;
}

int frp_nmpc_host_unregister(void *ptr)
{
    std::lock_guard<std::mutex> lock(g_reg.mtx);
    char *c = reinterpret_cast<char *>(ptr);
    for (size_t i = 0; i < g_reg.aliases.size(); i++)
        if (g_reg.aliases[i].ptr == c) { g_reg.aliases.erase(g_reg.aliases.begin() + (long)i); return FRP_OK; }
    for (size_t i = 0; i < g_reg.ranges.size(); i++)
        if (g_reg.ranges[i].base == c) {
            if (g_reg.ranges[i].refs > 1) { g_reg.ranges[i].refs--; return FRP_OK; }
            for (const HostRegistry::Alias &al : g_reg.aliases)
                if (al.owner == c) return FRP_ERR_ARG; // (sub-ranges registered through it are still in use)
            const hipError_t rc = hipHostUnregister(ptr);
            g_reg.ranges.erase(g_reg.ranges.begin() + (long)i);
            return rc == hipSuccess ? FRP_OK : FRP_ERR_HIP;
        }
    return FRP_ERR_ARG;
}

int frp_nmpc_host_registered(const void *ptr, size_t bytes)
{
    if (!ptr || !bytes) return 0;
    std::lock_guard<std::mutex> lock(g_reg.mtx);
    return g_reg.containing(reinterpret_cast<const char *>(ptr), bytes) ? 1 : 0;
}

// (known gap, left for a change of its own: this takes g_pipe.mtx but not g_async.mtx, so a pipelined batch may still be writing pages it unpins)
int frp_nmpc_host_unregister_all(void)
{
    // (a caller that lost track -- e.g. arrays garbage-collected without frp_nmpc_host_unregister -- starts over: no stale range may
    // survive to be taken for a new allocation at the same address)
    std::lock_guard<std::mutex> pipe_lock(g_pipe.mtx); // no host batch is in flight on the ranges while they go
    std::lock_guard<std::mutex> lock(g_reg.mtx);
    int rc = FRP_OK;
    for (const HostRegistry::Range &r : g_reg.ranges)
        if (hipHostUnregister(r.base) != hipSuccess) { (void)hipGetLastError(); rc = FRP_ERR_HIP; }
    g_reg.ranges.clear(); g_reg.aliases.clear();
    return rc;
}

int frp_nmpc_solve_batch_host(const frp_nmpc_batch *h, const frp_nmpc_options *opt)
{
    if (!batch_shape_ok(h)) return FRP_ERR_ARG;
    if (frp_nmpc_device_count() <= 0) return FRP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lock(g_pipe.mtx);
    // every chunk of this call runs on the kernel variants ONE launch of the whole batch would run on (the four-per-CU variants are
    // chosen by batch size and sum in another order): the plans do not depend on how the staging is cut (KernelArgs::variant_B --
    // an argument of the launch, not process state: concurrent frp_nmpc_solve_batch calls on other threads keep their own choice)
    int dev = 0;
    FRP_HIP(hipGetDevice(&dev));
    if (const int rc = g_pipe.ensure(dev); rc != FRP_OK) return rc;
    // (declared before the guard below: on an error path the kernels still writing the caller's registered memory are drained UNDER the
    // registry lock, so nobody unregisters -- unpins -- those pages while they are being written)
    std::lock_guard<std::mutex> reg_lock(g_reg.mtx);
    struct DirtyOnError { // every early return below leaves the slots in use: they are drained before the error is returned
        int rc = FRP_ERR_HIP;
        ~DirtyOnError() { if (rc != FRP_OK && g_pipe.ready) { g_pipe.drain_all(); } }
    } guard;
    // every array of the batch inside ranges the caller registered (frp_nmpc_host_register): no staging, see HostRegistry
    frp_nmpc_batch m;
    const bool mapped = g_reg.resolve(h, &m);
    const size_t N = h->N;
    // Chunks whose copies and solves overlap.  A small first chunk gets the GPU going while the rest is still being staged, the
    // later ones are large because a launch of fewer problems than two rounds of resident workgroups is inefficient: B / 16,
    // B / 4, then the rest in pieces of at most 4096 (measured on the 4096-problem batch, ms end to end: one chunk 2.54, three
    // equal ones 2.56, 256 + 1024 + 2816 2.09).
    size_t chunk = (size_t)h->B;
    std::vector<size_t> cb{0};
    if (h->B >= 4096 && !mapped) { // (registered buffers: one chunk, see the gather below)
        cb.push_back((size_t)h->B / 16);
        cb.push_back(cb.back() + (size_t)h->B / 4);
        const size_t rest = (size_t)h->B - cb.back(), nc = (rest + 4095) / 4096;
        chunk = (rest + nc - 1) / nc;
    }
    // chunk c covers the problems [cb[c], cb[c + 1]); FRP_HOST_SPLIT="n0,n1,..." gives explicit sizes, the rest uniform (the tests cut a batch with it)
    if (const char *e = getenv("FRP_HOST_SPLIT")) {
        cb.assign(1, 0);
        for (const char *q = e; *q && cb.back() < (size_t)h->B;) {
            char *end = nullptr; const long v = strtol(q, &end, 10);
            if (end == q || v <= 0) break;
            cb.push_back(std::min((size_t)h->B, cb.back() + (size_t)v));
            q = (*end == ',') ? end + 1 : end;
        }
    }
    while (cb.back() < (size_t)h->B) cb.push_back(std::min((size_t)h->B, cb.back() + chunk));
    const size_t nchunk = cb.size() - 1;
    for (size_t c = 0; c < nchunk; c++) chunk = std::max(chunk, cb[c + 1] - cb[c]); // (buffers are sized for the largest)
    const ChunkLayout largest(h, chunk);
    for (auto &s : g_pipe.slot) {
        int rc = grow(s.d_in, &s.h_in, s.in_bytes, largest.in_bytes);
        if (rc == FRP_OK) rc = grow(s.d_out, &s.h_out, s.out_bytes, largest.out_bytes);
        if (rc == FRP_OK) rc = grow(s.d_ws, nullptr, s.ws_bytes, frp::ws_bytes((int)chunk, h->N, h->MF));
        if (rc != FRP_OK) return rc;
    }
    // one wall-clock budget for the whole call: every chunk's launch stamps / reads the call's own origin word, zeroed here in front of
    // the first one (a chunk's queue header is its slot's, and a slot serves several chunks)
    frp::KernelArgs budget;
    if (!budget_args(opt ? opt->timeout : 0.0, &budget)) return FRP_ERR_ARG;
    if (budget.deadline) FRP_HIP(hipMemsetAsync(g_pipe.d_origin, 0, sizeof(unsigned long long), g_pipe.s_solve));
    auto drain = [&](size_t c) -> int { // chunk c's results: wait for its copy-out, unpack from the pinned block
        HostPipe::Slot &s = g_pipe.slot[c % HostPipe::NSLOT];
        FRP_HIP(hipEventSynchronize(s.e_out));
        if (mapped) return FRP_OK; // (the solver wrote the caller's arrays in place)
        const size_t b0 = cb[c];
        const ChunkLayout L(h, cb[c + 1] - b0);
        copy_pool().copy(h->z + b0 * N * 17, s.h_out, L.nb * N * 17 * sizeof(double));
        if (h->info) std::memcpy(h->info + b0 * FRP_INFO_STRIDE, s.h_out + L.info, L.nb * FRP_INFO_STRIDE * sizeof(double));
        const int *fi = reinterpret_cast<const int *>(s.h_out + L.flags);
        std::memcpy(h->exitflag + b0, fi, L.nb * sizeof(int));
        std::memcpy(h->iters + b0, fi + L.nb, L.nb * sizeof(int));
        return FRP_OK;
    };
    for (size_t c = 0; c < nchunk; c++) {
        HostPipe::Slot &s = g_pipe.slot[c % HostPipe::NSLOT];
        if (c >= HostPipe::NSLOT) { const int rc = drain(c - HostPipe::NSLOT); if (rc != FRP_OK) return rc; } // the slot's previous chunk has left it
        const size_t b0 = cb[c];
        const ChunkLayout L(h, cb[c + 1] - b0);
        // (measured, 4096 problems of configs[2] in the reference's 30-row layout, host link ~25 GB/s: the gather KERNEL in one chunk 2.03 ms,
        // in chunks 2.3-2.7 -- a resident gather block keeps the solver's persistent workgroups of the previous chunk off its CU --;
        // the copy engines (two strided copies for the parameter rows; since removed) 2.07-2.33 whatever the split; staging from pageable memory
        // 2.4-3.6.  The bound on that link is (28 MB in + 5.6 MB out) / 25 GB/s + the 0.85 ms solve = 2.0 ms without overlap.)
        if (mapped) {
            launch_gather(L, m, b0, (unsigned)std::min<size_t>(2048, (L.nfaces + 255) / 256), s.d_in, g_pipe.s_in); // (a thread per double in front of the ints)
            FRP_HIP(hipGetLastError());
        } else {
            std::memcpy(s.h_in, h->xinit + b0 * 9, L.nb * 9 * sizeof(double));
            copy_pool().copy(s.h_in + L.x0, h->x0 + b0 * N * 17, L.nb * N * 17 * sizeof(double));
            if (L.Md < L.M) copy_pool().pack_rows(s.h_in + L.params, h->params + b0 * N * L.np_h, L.nb * N, L.M, L.Md);
            else copy_pool().copy(s.h_in + L.params, h->params + b0 * N * L.np, L.nb * N * L.np * sizeof(double));
            if (h->nfaces) std::memcpy(s.h_in + L.nfaces, h->nfaces + b0 * N, L.nb * N * sizeof(int));
            if (h->model_per_problem) std::memcpy(s.h_in + L.models, h->model_per_problem + b0, L.nb * sizeof(int));
            FRP_HIP(hipMemcpyAsync(s.d_in, s.h_in, L.in_bytes, hipMemcpyHostToDevice, g_pipe.s_in));
        }
        FRP_HIP(hipEventRecord(s.e_in, g_pipe.s_in));
        frp_nmpc_batch d = *h;
        L.point_inputs(&d, s.d_in);
        d.order_hint = nullptr; // (a queue-order hint is not worth a copy here: the chunks are at most two rounds of resident workgroups)
        d.z = s.d_out; d.info = h->info ? s.d_out + L.info : nullptr;
        d.exitflag = reinterpret_cast<int *>(s.d_out + L.flags); d.iters = d.exitflag + L.nb;
        if (mapped) { d.z = m.z + b0 * N * 17; d.info = m.info ? m.info + b0 * FRP_INFO_STRIDE : nullptr; d.exitflag = m.exitflag + b0; d.iters = m.iters + b0; }
        FRP_HIP(hipStreamWaitEvent(g_pipe.s_solve, s.e_in, 0));
        {
            frp::KernelArgs ka;
            if (!fill_args(&d, opt, s.d_ws, s.ws_bytes, &ka)) return FRP_ERR_ARG;
            ka.variant_B = h->B;
            if (ka.deadline) ka.origin = g_pipe.d_origin;
            FRP_HIP(frp::launch_ipm(ka, g_pipe.s_solve));
        }
        FRP_HIP(hipEventRecord(s.e_solve, g_pipe.s_solve));
        if (mapped) { FRP_HIP(hipEventRecord(s.e_out, g_pipe.s_solve)); continue; }
        FRP_HIP(hipStreamWaitEvent(g_pipe.s_out, s.e_solve, 0));
        FRP_HIP(hipMemcpyAsync(s.h_out, s.d_out, L.out_bytes, hipMemcpyDeviceToHost, g_pipe.s_out));
        FRP_HIP(hipEventRecord(s.e_out, g_pipe.s_out));
    }
    for (size_t c = nchunk > HostPipe::NSLOT ? nchunk - HostPipe::NSLOT : 0; c < nchunk; c++) {
        const int rc = drain(c);
        if (rc != FRP_OK) return rc;
    }
    guard.rc = FRP_OK;
    return FRP_OK;
}

int frp_nmpc_solve_batch_host_begin(const frp_nmpc_batch *h, const frp_nmpc_options *opt, int *ticket)
{
    if (!ticket) return FRP_ERR_ARG;
    *ticket = -1;
    if (!batch_shape_ok(h)) return FRP_ERR_ARG;
    if (frp_nmpc_device_count() <= 0) return FRP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lock(g_async.mtx);
    int dev = 0;
    FRP_HIP(hipGetDevice(&dev));
    if (const int rc = g_async.ensure(dev); rc != FRP_OK) return rc;
    int si = -1;
    for (int i = 0; i < AsyncPipe::NSLOT; i++)
        if (!g_async.slot[i].busy) { si = i; break; }
    if (si < 0) return FRP_ERR_ARG; // (FRP_NMPC_HOST_INFLIGHT batches are out: wait for one)
    AsyncPipe::Slot &s = g_async.slot[si];
    std::lock_guard<std::mutex> reg_lock(g_reg.mtx);
    frp_nmpc_batch m;
    if (!g_reg.resolve(h, &m)) return FRP_ERR_ARG; // every array of a pipelined batch is registered (frp_nmpc_host_register): nothing is staged on this path
    const ChunkLayout L(h, (size_t)h->B);
    if (const int rc = grow(s.d_in, nullptr, s.in_bytes, L.in_bytes); rc != FRP_OK) return rc;
    if (const int rc = grow(s.d_ws, nullptr, s.ws_bytes, frp::ws_bytes(h->B, h->N, h->MF)); rc != FRP_OK) return rc;
    launch_gather(L, m, 0, AsyncPipe::GATHER_WGS, s.d_in, g_async.s_gather);
    FRP_HIP(hipGetLastError());
    FRP_HIP(hipEventRecord(s.e_in, g_async.s_gather));
    frp_nmpc_batch d = m; // (the solver writes the caller's arrays in place)
    L.point_inputs(&d, s.d_in);
    d.order_hint = nullptr;
    frp::KernelArgs ka;
    if (!fill_args(&d, opt, s.d_ws, s.ws_bytes, &ka)) return FRP_ERR_ARG;
    ka.slot_reserve = AsyncPipe::GATHER_WGS;
    FRP_HIP(hipStreamWaitEvent(g_async.s_solve, s.e_in, 0));
    FRP_HIP(frp::launch_ipm(ka, g_async.s_solve));
    FRP_HIP(hipEventRecord(s.e_done, g_async.s_solve));
    s.busy = true;
    *ticket = si;
    return FRP_OK;
}

int frp_nmpc_solve_batch_host_wait(int ticket)
{
    if (ticket < 0 || ticket >= AsyncPipe::NSLOT) return FRP_ERR_ARG;
    hipEvent_t ev;
    {
        std::lock_guard<std::mutex> lock(g_async.mtx);
        if (!g_async.ready || !g_async.slot[ticket].busy) return FRP_ERR_ARG;
        ev = g_async.slot[ticket].e_done;
    }
    const hipError_t rc = hipEventSynchronize(ev); // (outside the lock: another thread may begin the next batch meanwhile)
    std::lock_guard<std::mutex> lock(g_async.mtx);
    g_async.slot[ticket].busy = false;
    if (rc != hipSuccess) { fprintf(stderr, "[frp_nmpc] HIP error %s while waiting for a pipelined host batch\n", hipGetErrorString(rc)); return FRP_ERR_HIP; }
    return FRP_OK;
}

} // extern "C"
