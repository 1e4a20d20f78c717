// frp_flight_record.hip -- frp_nmpc.h section (14): the flight record.  Per-vehicle accumulators of what a fleet flew (tracking error,
// path length, speed, saturation, tick outcomes, state-machine states, first arrival) and the fleet's figures from them.  No reference
// counterpart; tests/flight_record_oracle.py is the executable statement, and this file agrees with it to the bit.
//
//   * samples / period / reset: one thread per vehicle, 256 per workgroup, no LDS, no barrier, no atomics: a vehicle reads and writes its
//     own rows alone.  The accumulators live in registers across the S samples; per sample a thread reads 48 bytes of trace, 24 of
//     command, a kind and (where given) a sat word.  Rows of neighbouring lanes are S * stride * 8 bytes apart, so the loads are not
//     coalesced -- at 4096 vehicles and S = 5 that is about 2 MB per call: the cost is the launch.
//   * summary: launch 1, one workgroup per FRP_FLIGHT_GROUP = 256 consecutive vehicles, writes one row of 90 eight-byte partials per
//     workgroup into the workspace; launch 2, ONE workgroup, thread t adds partial t of every row in row order and writes the result.
//     Nothing waits on another workgroup: the kernel boundary is the only ordering.
//     The two float sums have the header's order: v[i] += v[i + stride] for stride = 128 ... 1.  Strides 128 and 64 go through LDS
//     (v[i + stride] belongs to another wave); strides 32 ... 1 stay in wave 0, where lane i + stride's value comes by __shfl_down --
//     lanes >= stride compute values nobody reads.  The same additions of the same operands, so the same bits as the LDS tree.
//     Integers, maxima and the minimum do not depend on the order: a shuffle reduction per wave, then the four waves through LDS.  The
//     histogram bins are LDS integer atomics.
//   * No contraction in this file (the build passes -ffp-contract=off as well): dx * dx + dy * dy is two products and a sum.
//   * Every index is b < B, s < S as the entry point checked them (B * S * stride fits an int; offsets are formed in size_t); a bin is
//     <= n_edges <= 64, a state-histogram index is tested to be 0 ... 5 before it is used.
//   * Every store is a plain C++ store from a vector lane; no inline assembly.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_fleet.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace flight {

// (by name, not the whole namespace: THREADS and ROW below are this unit's own)
using fleet::blocks_for;
using fleet::device_ok;
using fleet::finite_d;
using fleet::launch;

constexpr int THREADS = FRP_FLIGHT_GROUP;
static_assert(THREADS == fleet::THREADS, "the summary's group is the workgroup fleet::blocks_for and fleet::launch count in");
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int NI = FRP_FLIGHT_SUM_INTS;
constexpr int NBIN = FRP_FLIGHT_MAX_EDGES + 1;
constexpr int NF = FRP_FLIGHT_SUM_F64;
constexpr int ROW = NI + NBIN + NF; // eight-byte words per workgroup in the workspace: the integers, the bins, the doubles
static_assert(ROW <= THREADS, "the second launch takes one partial per thread");
static_assert(sizeof(long long) == 8 && sizeof(double) == 8, "one row is ROW eight-byte words");

__device__ inline bool finite3(const double *v) { return finite_d(v[0]) && finite_d(v[1]) && finite_d(v[2]); }
__device__ inline double sq3(double x, double y, double z) { return (x * x + y * y) + z * z; }

__global__ __launch_bounds__(THREADS) void samples_kernel(frp_nmpc_flight_record r, int S, const double *trace, int stride, const double *cmd,
                                                          const int *kind, const int *sat, const int *active)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= r.B) return;
    if (active && active[b] == 0) return;
    double p0[3];
#pragma unroll
    for (int i = 0; i < 3; i++) p0[i] = r.p_prev[(size_t)b * 3 + i];
    int have = r.have_prev[b];
    double tmax = r.track_max2[b], tsum = r.track_sum2[b], plen = r.path_len[b], vmax = r.speed_max2[b];
    int tn = r.track_n[b], n = r.samples[b], flown = r.flown[b], bad = r.bad[b], satn = r.sat_samples[b], bits = r.sat_bits[b];
    for (int s = 0; s < S; s++) {
        const size_t bs = (size_t)b * S + s;
        const double *row = trace + bs * stride;
        const double *c = cmd + bs * FRP_COMMAND_STRIDE;
        const double p1[3] = {row[0], row[1], row[2]}, v1[3] = {row[3], row[4], row[5]};
        const int k = kind[bs];
        const bool tracked = k == FRP_COMMAND_TRAJ || k == FRP_COMMAND_END;
        n += 1;
        if (sat) {
            const int w = sat[bs];
            bits |= w;
            if (w & FRP_FLIGHT_SAT_MASK) satn += 1;
        }
        const double cp[3] = {tracked ? c[0] : 0.0, tracked ? c[1] : 0.0, tracked ? c[2] : 0.0}; // (read only where it counts)
        const bool is_bad = have && (!finite3(p0) || !finite3(p1) || !finite3(v1) || !finite3(cp));
        if (is_bad) {
            bad += 1;
        } else {
            if (have) {
                plen += sqrt(sq3(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]));
                if (tracked) {
                    const double e2 = sq3(p0[0] - cp[0], p0[1] - cp[1], p0[2] - cp[2]);
                    tsum += e2;
                    tmax = e2 > tmax ? e2 : tmax;
                    tn += 1;
                }
            }
            const double v2 = sq3(v1[0], v1[1], v1[2]);
            vmax = v2 > vmax ? v2 : vmax;
        }
        if (tracked) flown += 1;
#pragma unroll
        for (int i = 0; i < 3; i++) p0[i] = p1[i];
        have = 1;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) r.p_prev[(size_t)b * 3 + i] = p0[i];
    r.have_prev[b] = have;
    r.track_max2[b] = tmax; r.track_sum2[b] = tsum; r.path_len[b] = plen; r.speed_max2[b] = vmax;
    r.track_n[b] = tn; r.samples[b] = n; r.flown[b] = flown; r.bad[b] = bad; r.sat_samples[b] = satn; r.sat_bits[b] = bits;
}

__device__ inline int result_bin(int result) { return result <= 1 && result >= -3 ? 1 - result : FRP_FLIGHT_RESULT_BINS - 1; }

__global__ __launch_bounds__(THREADS) void period_kernel(frp_nmpc_flight_record r, const int *fsm_state, const int *gate, const int *result,
                                                         const int *exit_code, const int *active)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= r.B) return;
    if (active && active[b] == 0) return;
    const int periods = r.periods[b] + 1;
    r.periods[b] = periods;
    if (gate[b] == FRP_TICK_RUN) {
        r.ticks_run[b] += 1;
        if (exit_code[b] == 1) r.ticks_converged[b] += 1;
    }
    const int res = result[b], st = fsm_state[b];
    r.result_hist[(size_t)b * FRP_FLIGHT_RESULT_BINS + result_bin(res)] += 1;
    if (st >= 0 && st < FRP_FLIGHT_STATE_BINS) r.state_hist[(size_t)b * FRP_FLIGHT_STATE_BINS + st] += 1;
    if (res == 0 && r.first_arrival[b] < 0) r.first_arrival[b] = periods - 1;
}

__global__ __launch_bounds__(THREADS) void reset_kernel(frp_nmpc_flight_record r, const int *mask, const double *x)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= r.B) return;
    if (mask && mask[b] == 0) return;
    r.track_max2[b] = 0.0; r.track_sum2[b] = 0.0; r.path_len[b] = 0.0; r.speed_max2[b] = 0.0;
    r.track_n[b] = 0; r.samples[b] = 0; r.flown[b] = 0; r.bad[b] = 0; r.sat_samples[b] = 0; r.sat_bits[b] = 0;
    r.periods[b] = 0; r.ticks_run[b] = 0; r.ticks_converged[b] = 0;
#pragma unroll
    for (int i = 0; i < FRP_FLIGHT_RESULT_BINS; i++) r.result_hist[(size_t)b * FRP_FLIGHT_RESULT_BINS + i] = 0;
#pragma unroll
    for (int i = 0; i < FRP_FLIGHT_STATE_BINS; i++) r.state_hist[(size_t)b * FRP_FLIGHT_STATE_BINS + i] = 0;
    r.first_arrival[b] = -1;
    if (x) {
#pragma unroll
        for (int i = 0; i < 3; i++) r.p_prev[(size_t)b * 3 + i] = x[(size_t)b * FRP_VEHICLE_STATE + i];
        r.have_prev[b] = 1;
    } else {
        r.have_prev[b] = 0;
    }
}

__device__ inline long long wave_sum(long long v)
{
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_down(v, d, WAVE);
    return v; // (lane 0 holds the wave's sum)
}

__device__ inline double wave_max(double v)
{
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const double o = __shfl_down(v, d, WAVE);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline double wave_min(double v)
{
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const double o = __shfl_down(v, d, WAVE);
        v = o < v ? o : v;
    }
    return v;
}

// launch 1: the partials of workgroup g over vehicles 256 g ... 256 g + 255 into row g of the workspace
__global__ __launch_bounds__(THREADS) void summary_partial_kernel(frp_nmpc_flight_record r, const double *min_clear, const int *hits, const int *mask,
                                                                  int n_edges, const double *edges, long long *ws)
{
    __shared__ long long wi[WAVES][NI];
    __shared__ double wf[WAVES][4];
    __shared__ double tree[2][THREADS];
    __shared__ unsigned int bins[NBIN];
    const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    const int b = blockIdx.x * THREADS + t;
    const bool sel = b < r.B && (!mask || mask[b] != 0);
    if (t < NBIN) bins[t] = 0u;
    __syncthreads();

    long long vi[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) vi[i] = 0;
    double tmax = 0.0, vmax = 0.0, pmax = 0.0, cmin = INFINITY, tsum = 0.0, plen = 0.0;
    if (sel) {
        const int fa = r.first_arrival[b], nbad = r.bad[b], tn = r.track_n[b];
        vi[FRP_FLIGHT_I_SELECTED] = 1;
        vi[FRP_FLIGHT_I_ARRIVED] = fa >= 0;
        vi[FRP_FLIGHT_I_WITH_BAD] = nbad > 0;
        vi[FRP_FLIGHT_I_WITH_HITS] = hits ? hits[b] > 0 : 0;
        vi[FRP_FLIGHT_I_SAMPLES] = r.samples[b];
        vi[FRP_FLIGHT_I_FLOWN] = r.flown[b];
        vi[FRP_FLIGHT_I_TRACK_N] = tn;
        vi[FRP_FLIGHT_I_BAD] = nbad;
        vi[FRP_FLIGHT_I_SAT_SAMPLES] = r.sat_samples[b];
        vi[FRP_FLIGHT_I_PERIODS] = r.periods[b];
        vi[FRP_FLIGHT_I_TICKS_RUN] = r.ticks_run[b];
        vi[FRP_FLIGHT_I_TICKS_CONVERGED] = r.ticks_converged[b];
#pragma unroll
        for (int i = 0; i < FRP_FLIGHT_RESULT_BINS; i++) vi[FRP_FLIGHT_I_RESULT + i] = r.result_hist[(size_t)b * FRP_FLIGHT_RESULT_BINS + i];
        vi[FRP_FLIGHT_I_ARRIVAL_SUM] = fa >= 0 ? fa : 0;
        tmax = r.track_max2[b]; vmax = r.speed_max2[b]; plen = r.path_len[b]; tsum = r.track_sum2[b];
        pmax = plen;
        if (min_clear) cmin = min_clear[b];
        if (tn > 0) {
            const double m = tsum / (double)tn;
            int bin = 0;
            for (int j = 0; j < n_edges; j++) bin += edges[j] <= m ? 1 : 0;
            atomicAdd(&bins[bin], 1u);
        }
    }
    // integers, maxima, the minimum: any order
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const long long s = wave_sum(vi[i]);
        if (lane == 0) wi[wave][i] = s;
    }
    {
        // (a maximum starts at 0, the minimum at +inf, and only v > max / v < min move them: a NaN never enters)
        const double a = wave_max(tmax > 0.0 ? tmax : 0.0), c = wave_max(vmax > 0.0 ? vmax : 0.0), d = wave_max(pmax > 0.0 ? pmax : 0.0);
        const double e = wave_min(cmin < INFINITY ? cmin : INFINITY);
        if (lane == 0) { wf[wave][0] = a; wf[wave][1] = c; wf[wave][2] = d; wf[wave][3] = e; }
    }
    // the two sums: the header's tree
    tree[0][t] = tsum;
    tree[1][t] = plen;
    __syncthreads();
    if (t < 128) { tree[0][t] += tree[0][t + 128]; tree[1][t] += tree[1][t + 128]; }
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    if (wave == 0) {
        s0 = tree[0][t] + tree[0][t + 64];
        s1 = tree[1][t] + tree[1][t + 64];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            s0 += __shfl_down(s0, d, WAVE);
            s1 += __shfl_down(s1, d, WAVE);
        }
    }
    long long *row = ws + (size_t)blockIdx.x * ROW;
    if (t < NI) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += wi[w][t];
        row[t] = s;
    } else if (t < NI + NBIN) {
        row[t] = (long long)bins[t - NI];
    }
    double *rowf = reinterpret_cast<double *>(row + NI + NBIN);
    if (t == 0) {
        rowf[FRP_FLIGHT_F_TRACK_SUM2] = s0;
        rowf[FRP_FLIGHT_F_PATH_SUM] = s1;
    }
    if (t >= WAVE && t < WAVE + 4) {
        const int i = t - WAVE;
        double v = wf[0][i];
#pragma unroll
        for (int w = 1; w < WAVES; w++) v = i < 3 ? (wf[w][i] > v ? wf[w][i] : v) : (wf[w][i] < v ? wf[w][i] : v);
        rowf[i] = v;
    }
}
static_assert(FRP_FLIGHT_F_TRACK_MAX2 == 0 && FRP_FLIGHT_F_SPEED_MAX2 == 1 && FRP_FLIGHT_F_PATH_MAX == 2 && FRP_FLIGHT_F_MIN_CLEAR == 3 &&
              FRP_FLIGHT_F_TRACK_SUM2 == 4 && FRP_FLIGHT_F_PATH_SUM == 5, "the partial row's doubles are out_f's");

// launch 2, ONE workgroup: thread t adds partial t of rows 0 ... G - 1 in that order
__global__ __launch_bounds__(THREADS) void summary_final_kernel(int G, int n_edges, const long long *ws, long long *out_i, double *out_f, long long *hist)
{
    const int t = threadIdx.x;
    if (t < NI + NBIN) {
        long long s = 0;
        for (int g = 0; g < G; g++) s += ws[(size_t)g * ROW + t];
        if (t < NI) out_i[t] = s;
        else if (t - NI <= n_edges) hist[t - NI] = s;
    } else if (t < ROW) {
        const int i = t - (NI + NBIN);
        const bool is_sum = i >= FRP_FLIGHT_F_TRACK_SUM2, is_min = i == FRP_FLIGHT_F_MIN_CLEAR;
        double v = is_min ? (double)INFINITY : 0.0;
        for (int g = 0; g < G; g++) {
            const double p = reinterpret_cast<const double *>(ws)[(size_t)g * ROW + t];
            if (is_sum) v += p;
            else if (is_min) v = p < v ? p : v;
            else v = p > v ? p : v;
        }
        out_f[i] = v;
    }
}

static bool complete(const frp_nmpc_flight_record *r)
{
    return r && r->B >= 0 && r->p_prev && r->have_prev && r->track_max2 && r->track_sum2 && r->track_n && r->path_len && r->speed_max2 && r->samples &&
           r->flown && r->bad && r->sat_samples && r->sat_bits && r->periods && r->ticks_run && r->ticks_converged && r->result_hist && r->state_hist &&
           r->first_arrival;
}

} // namespace flight
} // namespace frp

extern "C" {

int frp_nmpc_flight_record_samples(const frp_nmpc_flight_record *rec, int S, const double *trace, int stride, const double *cmd, const int *kind,
                                   const int *sat, const int *active, void *stream)
{
    using namespace frp::flight;
    if (!complete(rec) || !trace || !cmd || !kind || S < 1 || stride < 6) return FRP_ERR_ARG;
    if ((long long)rec->B * S > 0x7fffffffLL || (long long)rec->B * S * stride > 0x7fffffffLL) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (rec->B == 0) return FRP_OK;
    return launch(samples_kernel, blocks_for(rec->B), stream, *rec, S, trace, stride, cmd, kind, sat, active);
}

int frp_nmpc_flight_record_period(const frp_nmpc_flight_record *rec, const int *fsm_state, const int *gate, const int *result,
                                  const int *exit_code, const int *active, void *stream)
{
    using namespace frp::flight;
    if (!complete(rec) || !fsm_state || !gate || !result || !exit_code) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (rec->B == 0) return FRP_OK;
    return launch(period_kernel, blocks_for(rec->B), stream, *rec, fsm_state, gate, result, exit_code, active);
}

int frp_nmpc_flight_record_reset(const frp_nmpc_flight_record *rec, const int *mask, const double *x, void *stream)
{
    using namespace frp::flight;
    if (!complete(rec)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (rec->B == 0) return FRP_OK;
    return launch(reset_kernel, blocks_for(rec->B), stream, *rec, mask, x);
}

size_t frp_nmpc_flight_summary_workspace_bytes(int B)
{
    using namespace frp::flight;
    if (B < 0) return 0;
    const size_t G = blocks_for(B);
    return (G > 0 ? G : 1) * ROW * sizeof(long long);
}

int frp_nmpc_flight_summary(const frp_nmpc_flight_record *rec, const double *min_clear, const int *hits, const int *mask, int n_edges,
                            const double *edges, long long *out_i, double *out_f, long long *hist, void *workspace, size_t workspace_bytes,
                            void *stream)
{
    using namespace frp::flight;
    if (!complete(rec) || !out_i || !out_f || !hist || !workspace) return FRP_ERR_ARG;
    if (n_edges < 0 || n_edges > FRP_FLIGHT_MAX_EDGES || (n_edges > 0 && !edges) || (min_clear == nullptr) != (hits == nullptr)) return FRP_ERR_ARG;
    if (workspace_bytes < frp_nmpc_flight_summary_workspace_bytes(rec->B)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    const unsigned G = blocks_for(rec->B);
    long long *ws = static_cast<long long *>(workspace);
    if (G > 0 && launch(summary_partial_kernel, G, stream, *rec, min_clear, hits, mask, n_edges, edges, ws) != FRP_OK) return FRP_ERR_HIP;
    return launch(summary_final_kernel, 1, stream, (int)G, n_edges, ws, out_i, out_f, hist);
}

} // extern "C"
