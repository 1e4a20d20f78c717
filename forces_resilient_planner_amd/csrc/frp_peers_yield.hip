// frp_peers_yield.hip -- frp_nmpc.h section (20): right of way.  An order among vehicles, the peer boxes that respect it, and the rule that
// makes the planner that has to yield stop, wait and take up its goal again.  No reference counterpart; tests/right_of_way_oracle.py is
// the executable statement and this file agrees with it to the bit (built with -ffp-contract=off, like the other two units of the peers).
//
//   * ranked boxes: frp_peers_boxes.hip's kernel -- one wavefront per planner, four per workgroup, select_near, the two ballot passes, the
//     box list in global memory -- with one test in front of peer_box (frp_peers.hpp): a centre other than the peer's position is taken
//     only where the peer outranks the planner.  The first pass also counts the kept boxes of outranking peers; the smallest d2 to an
//     outranking peer is the key of the first such lane of the kept list, which select_near leaves ascending.  LDS: the selection's 52224
//     bytes per workgroup; no __syncthreads.
//   * hold and release: one thread per planner, no LDS, no atomics; every planner reads and writes its own elements alone.
//   * Every store is a plain C++ store from a vector lane; no inline assembly.
#include "frp_peers.hpp"

namespace frp {
namespace peers {

// does q outrank b (priority NULL: all zero)
__device__ inline bool outranks(const int *priority, int q, int b)
{
    const int pq = priority ? priority[q] : 0, pb = priority ? priority[b] : 0;
    return pq > pb || (pq == pb && q < b);
}

// peer_box of centre t where the rank lets it through: `up` <- does the peer outrank b
__device__ inline int ranked_box(const frp_nmpc_peers &p, const frp_nmpc_peers_box_view &v, const double *pos, int stride, const int *priority, int b, const int *kp,
                                 int nc, int t, double inv, const double own[3], int lo[3], int hi[3], bool &up)
{
    const int peer = kp[t / nc];
    up = peer >= 0 && peer < p.B && outranks(priority, peer, b);
    if (t % nc != 0 && !up) return 0;
    return peer_box(p, v, pos, stride, kp, nc, t, inv, own, lo, hi);
}

__global__ __launch_bounds__(THREADS) void boxes_ranked_kernel(frp_nmpc_peers p, frp_nmpc_peers_box_view v, const double *pos, int stride, double R2, double inv,
                                                               const int *priority, int *outrank_boxes, double *outrank_d2)
{
    __shared__ double cand_d[WAVES][CAND];
    __shared__ int cand_p[WAVES][CAND];
    __shared__ double kept_d[WAVES][NEAR];
    __shared__ int kept_p[WAVES][NEAR];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const int b = blockIdx.x * WAVES + wave; // (uniform in the wave)
    if (b >= p.B) return;
    int *kp = kept_p[wave];
    int seen = 0;
    const int m = select_near(p, pos, stride, R2, b, lane, cand_d[wave], cand_p[wave], kept_d[wave], kp, seen);
    const int nc = 1 + v.K, slots = m * nc;
    const double *me = pos + (size_t)b * stride;
    const double own[3] = {voxel_f(me[0], v.origin[0], inv), voxel_f(me[1], v.origin[1], inv), voxel_f(me[2], v.origin[2], inv)};
    // lane = kept peer (m <= NEAR == WAVE): the nearest one that outranks b
    const bool above = lane < m && kp[lane] >= 0 && kp[lane] < p.B && outranks(priority, kp[lane], b);
    const unsigned long long above_mask = __ballot(above);
    const int first_above = above_mask ? (int)__ffsll((long long)above_mask) - 1 : -1;
    int n = 0, dropped = 0, n_above = 0;
    for (int t0 = 0; t0 < slots; t0 += WAVE) {
        int lo[3], hi[3];
        bool up = false;
        const int r = t0 + lane < slots ? ranked_box(p, v, pos, stride, priority, b, kp, nc, t0 + lane, inv, own, lo, hi, up) : 0;
        n += (int)__popcll(__ballot(r == 1));
        n_above += (int)__popcll(__ballot(r == 1 && up));
        dropped += (int)__popcll(__ballot(r == -1));
    }
    const bool fits = n <= v.Q;
    if (fits) {
        int at0 = 0;
        for (int t0 = 0; t0 < slots; t0 += WAVE) {
            int lo[3], hi[3];
            bool up = false;
            const bool ok = t0 + lane < slots && ranked_box(p, v, pos, stride, priority, b, kp, nc, t0 + lane, inv, own, lo, hi, up) == 1;
            const unsigned long long mask = __ballot(ok);
            const int at = at0 + (int)__popcll(mask & ((1ull << lane) - 1ull));
            if (ok && at >= 0 && at < v.Q) {
                int *dst = v.boxes + ((size_t)b * v.Q + at) * 6;
                dst[0] = lo[0]; dst[1] = lo[1]; dst[2] = lo[2]; dst[3] = hi[0]; dst[4] = hi[1]; dst[5] = hi[2];
            }
            at0 += (int)__popcll(mask);
        }
    }
    if (lane == 0) {
        v.count[b] = fits ? n : -n;
        v.overflow[b] = seen > NEAR ? 1 : 0;
        v.dropped_own[b] = dropped;
        outrank_boxes[b] = n_above;
        outrank_d2[b] = first_above >= 0 ? kept_d[wave][first_above] : R2;
    }
}

// frp_nmpc.h section (20), "hold and release", in its order
__global__ __launch_bounds__(THREADS) void yield_step_kernel(frp_nmpc_yield y, frp_nmpc_fsm f)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= y.B) return;
    const size_t b3 = 3 * (size_t)b;
    const bool was_holding = y.holding[b] != 0;
    const bool fresh_in = y.fresh_in && y.fresh_in[b] != 0;
    int fresh = 0;
    if (fresh_in) {
        const double *g = y.goal_in + b3;
        double *dst = was_holding ? y.held_goal + b3 : y.goal + b3;
        dst[0] = g[0]; dst[1] = g[1]; dst[2] = g[2];
        fresh = was_holding ? 0 : 1;
    }
    if (!was_holding) {
        if (!fresh_in && y.astar_status[b] == FRP_ASTAR_NO_PATH && y.outrank_boxes[b] > 0 && f.state[b] != FRP_FSM_EXEC_TRAJ) {
            const double *od = y.state + 9 * (size_t)b;
            if (!finite3(od[0], od[1], od[2]) || !finite3(od[3], od[4], od[5])) {
                y.bad[b] += 1;
            } else {
                const double lead = sqrt(sq3(od[3], od[4], od[5])) / (2.0 * y.a_brake);
                const double *e = f.end_pt + b3;
                double *h = y.held_goal + b3, *c = y.cmd_end_pt + b3;
                h[0] = e[0]; h[1] = e[1]; h[2] = e[2];
                c[0] = od[0] + od[3] * lead; c[1] = od[1] + od[4] * lead; c[2] = od[2] + od[5] * lead;
                y.astar_status[b] = 0;
                f.have_target[b] = 0;
                f.state[b] = FRP_FSM_WAIT_TARGET;
                f.exec_mpc[b] = 0;
                f.plan_fail_count[b] = 0;
                f.have_traj[b] = 0;
                if (y.fleet_have_traj) y.fleet_have_traj[b] = 0;
                f.cmd_status[b] = FRP_CMD_PUB_END;
                f.pub_end[b] = 1;
                y.holding[b] = 1;
                y.holds[b] += 1;
                y.hold_age[b] = 0;
                y.clear_count[b] = 0;
            }
        }
    } else {
        const int age = y.hold_age[b] + 1;
        y.hold_age[b] = age;
        y.hold_periods[b] += 1;
        if (age > y.longest_hold[b]) y.longest_hold[b] = age;
        const bool clear = y.outrank_d2[b] > y.r_release * y.r_release || y.outrank_boxes[b] == 0;
        const int cc = clear ? y.clear_count[b] + 1 : 0;
        y.clear_count[b] = cc;
        const bool timeout = cc < y.n_clear && age >= y.hold_timeout;
        if (cc >= y.n_clear || timeout) {
            const double *h = y.held_goal + b3;
            double *g = y.goal + b3;
            g[0] = h[0]; g[1] = h[1]; g[2] = h[2];
            fresh = 1;
            y.holding[b] = 0;
            y.releases[b] += 1;
            if (timeout) y.timeouts[b] += 1;
        }
    }
    y.fresh[b] = fresh;
}

__global__ __launch_bounds__(THREADS) void yield_reset_kernel(frp_nmpc_yield y, const int *mask)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= y.B) return;
    if (mask && mask[b] == 0) return;
    y.holding[b] = 0; y.clear_count[b] = 0; y.hold_age[b] = 0; y.fresh[b] = 0;
    y.holds[b] = 0; y.releases[b] = 0; y.timeouts[b] = 0; y.hold_periods[b] = 0; y.longest_hold[b] = 0; y.bad[b] = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        y.held_goal[3 * (size_t)b + k] = 0.0;
        y.goal[3 * (size_t)b + k] = 0.0;
    }
}

// y's own arrays
static bool yield_own_ok(const frp_nmpc_yield *y)
{
    return y && y->B >= 1 && y->holding && y->clear_count && y->hold_age && y->held_goal && y->goal && y->fresh && y->holds && y->releases && y->timeouts &&
           y->hold_periods && y->longest_hold && y->bad;
}

} // namespace peers
} // namespace frp

extern "C" {

int frp_nmpc_peers_boxes_ranked(const frp_nmpc_peers *p, const frp_nmpc_peers_box_view *v, const double *pos, int stride, const int *priority,
                                int *outrank_boxes, double *outrank_d2, void *stream)
{
    using namespace frp::peers;
    if (!boxes_ok(p, v, pos, stride) || !outrank_boxes || !outrank_d2) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (p->B == 0) return FRP_OK;
    return launch(boxes_ranked_kernel, (unsigned)((p->B + WAVES - 1) / WAVES), stream, *p, *v, pos, stride, p->R * p->R, 1.0 / v->resolution, priority, outrank_boxes,
                  outrank_d2);
}

int frp_nmpc_yield_step(const frp_nmpc_yield *y, const frp_nmpc_fsm *f, void *stream)
{
    using namespace frp::peers;
    if (!yield_own_ok(y) || !f || f->B != y->B) return FRP_ERR_ARG;
    if (!f->state || !f->have_target || !f->have_traj || !f->exec_mpc || !f->plan_fail_count || !f->cmd_status || !f->pub_end || !f->end_pt) return FRP_ERR_ARG;
    if (y->n_clear < 1 || y->hold_timeout < 1 || !non_negative(y->r_release) || !(y->a_brake > 0.0)) return FRP_ERR_ARG;
    if (!y->state || !y->astar_status || !y->outrank_boxes || !y->outrank_d2 || !y->cmd_end_pt || (y->goal_in == nullptr) != (y->fresh_in == nullptr)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(yield_step_kernel, blocks_for(y->B), stream, *y, *f);
}

int frp_nmpc_yield_reset(const frp_nmpc_yield *y, const int *mask, void *stream)
{
    using namespace frp::peers;
    if (!yield_own_ok(y)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(yield_reset_kernel, blocks_for(y->B), stream, *y, mask);
}

} // extern "C"
