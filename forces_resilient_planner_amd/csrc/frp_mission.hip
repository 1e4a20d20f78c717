// frp_mission.hip -- frp_nmpc.h section (17): per-vehicle mission state on the device -- which goal comes next, whether the last one was
// reached, and the period's clock.  tests/mission_oracle.py is the statement: every product and sum below is written in its order and
// rounded on its own; there is no transcendental here, so the device and the oracle agree to the bit.
//
//   * step_kernel: one wavefront per vehicle, four per workgroup of 256 -- the shape of frp_occmap_check.hip's check_surround_kernel,
//     because the occupancy probe of a drawn goal is that unit's surround_free (frp_occmap_check.hpp), which takes a whole wavefront
//     and which EVERY lane has to enter.  So every lane of a wave loads the same words (one address per wave: a broadcast) and computes
//     the same decisions and the same candidate -- integer mixing, a few dozen instructions -- and all 64 lanes reach every
//     surround_free call together; the integer inputs of the branches go through readfirstlane, so those branches are scalar.
//   * Lane 0 does the bookkeeping, with plain stores; nothing that was stored is read again in the launch.
//   * A vehicle that is DONE leaves after its phase; one that is FLYING and on time after phase, clock, t_mark and have_target; one
//     inside its dwell after phase, clock and t_mark.  Each stores fresh = 0 and nothing else.
//   * The generator is frp_disturbance.hpp's as it is (mix, stream_key); the uniform is section (16)'s one line with a 64-bit index.
//   * Every index is checked: b < B, a waypoint index inside 0 ... route_len - 1 <= W - 1 (a route_len outside 1 ... W ends the
//     vehicle's mission instead of being used), the probe inside the map (surround_free's own tests).  Offsets are formed in size_t.
//   * No LDS, no atomics, no waiting between workgroups, no inline assembly.
//   * clock_kernel: one thread.  reset_kernel: one thread per vehicle.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_disturbance.hpp"
#include "frp_occmap_check.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace mission {

using disturbance::mix;
using disturbance::stream_key;
using fleet::finite_d;
using fleet::non_negative;

// what the step reads beside its own struct
struct In {
    const int *have_odom, *have_target;
    const double *end_pt, *state, *clock;
};

// u(h, j) in [0, 1) (frp_nmpc.h section 16): the quotient is exact
__device__ inline double uniform(unsigned long long h, unsigned long long j) { return (double)(mix(h + j) >> 11) / 9007199254740992.0; }

__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(256) void step_kernel(frp_nmpc_mission m, In in, occmap::Geo g, occmap::Half hf, const uint32_t *plane)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t b = (size_t)blockIdx.x * 4 + wave;
    if (b >= (size_t)m.B) return;
    int phase = uni(m.phase[b]);
    if (phase != FRP_MISSION_FLYING && phase != FRP_MISSION_IDLE) { // DONE
        if (lane == 0) m.fresh[b] = 0;
        return;
    }
    const double now = in.clock[0];
    double t_mark = m.t_mark[b];
    bool due = false, moved = false;
    if (phase == FRP_MISSION_FLYING) {
        if (uni(in.have_target[b]) == 0) { // the state machine let go of the target: reached, or dropped
            const double dx = in.state[b * 9] - in.end_pt[b * 3], dy = in.state[b * 9 + 1] - in.end_pt[b * 3 + 1], dz = in.state[b * 9 + 2] - in.end_pt[b * 3 + 2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= m.arrive_radius * m.arrive_radius) {
                const double lt = now - t_mark;
                if (lane == 0) {
                    m.reached[b] = m.reached[b] + 1;
                    m.leg_time_sum[b] = m.leg_time_sum[b] + lt;
                    if (m.leg_time_max[b] < lt) m.leg_time_max[b] = lt;
                }
            } else if (lane == 0) {
                m.dropped[b] = m.dropped[b] + 1;
            }
            phase = FRP_MISSION_IDLE; t_mark = now; moved = true;
        } else if (m.leg_timeout > 0.0 && now - t_mark > m.leg_timeout) { // abandoned: the next goal in this same call
            if (lane == 0) m.abandoned[b] = m.abandoned[b] + 1;
            phase = FRP_MISSION_IDLE; t_mark = now - m.dwell; moved = true; due = true;
        }
    }
    int fresh = 0;
    if (phase == FRP_MISSION_IDLE && (due || now - t_mark >= m.dwell) && uni(in.have_odom[b]) != 0) {
        const int leg = uni(m.leg[b]);
        const int j = leg + 1;
        double pt[3] = {0.0, 0.0, 0.0};
        bool have = false;
        if (m.route) { // route mode
            const int n = uni(m.route_len[b]);
            if (n < 1 || n > m.W || j < 0 || (!m.loop && j >= n)) {
                phase = FRP_MISSION_DONE; moved = true;
            } else {
                const double *w = m.route + ((size_t)b * (size_t)m.W + (size_t)(m.loop ? j % n : j)) * 3;
                pt[0] = w[0]; pt[1] = w[1]; pt[2] = w[2];
                have = true;
            }
        } else { // random mode
            const int tries = uni(m.tries[b]);
            const double px = in.state[b * 9], py = in.state[b * 9 + 1];
            const double min2 = m.min_dist * m.min_dist, max2 = m.max_dist * m.max_dist;
            const double wx = m.goal_box[1] - m.goal_box[0], wy = m.goal_box[3] - m.goal_box[2];
            const unsigned long long h = mix(stream_key((unsigned long long)m.seed, (unsigned long long)m.id0 + (unsigned long long)b, (unsigned long long)(long long)j) +
                                             (unsigned long long)FRP_MISSION_TAG);
            for (int i = 0; i < m.R && !have; i++) {
                const unsigned long long c = (unsigned long long)(long long)tries + (unsigned long long)i;
                const double x = m.goal_box[0] + uniform(h, 2ULL * c) * wx, y = m.goal_box[2] + uniform(h, 2ULL * c + 1ULL) * wy;
                const double dx = x - px, dy = y - py;
                const double d2 = dx * dx + dy * dy;
                bool ok = d2 >= min2 && d2 <= max2;
                if (ok && plane) ok = occmap::surround_free(g, hf, x, y, m.z_goal, nullptr, plane, lane); // (the same `ok` in every lane: all 64 enter)
                if (ok) { pt[0] = x; pt[1] = y; pt[2] = m.z_goal; have = true; }
            }
            if (!have && lane == 0) {
                m.blocked[b] = m.blocked[b] + 1;
                m.tries[b] = tries + m.R;
            }
        }
        if (have) {
            if (lane == 0) {
                m.leg[b] = j;
                m.tries[b] = 0;
                m.issued[b] = m.issued[b] + 1;
                m.goal[b * 3] = pt[0]; m.goal[b * 3 + 1] = pt[1]; m.goal[b * 3 + 2] = pt[2];
            }
            phase = FRP_MISSION_FLYING; t_mark = now; moved = true;
            fresh = 1;
        }
    }
    if (lane == 0) {
        m.fresh[b] = fresh;
        if (moved) { m.phase[b] = phase; m.t_mark[b] = t_mark; }
    }
}

__global__ void clock_kernel(long long *k, double t0, double period, double dt, int n, double *clock, int advance)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long k0 = k[0];
    const double base = t0 + (double)k0 * period;
    for (int j = 0; j < n; j++) clock[j] = base + dt * (double)j;
    k[0] = (long long)((unsigned long long)k0 + (unsigned long long)advance);
}

__global__ __launch_bounds__(fleet::THREADS) void reset_kernel(frp_nmpc_mission m, const int *mask)
{
    const int b = blockIdx.x * fleet::THREADS + threadIdx.x;
    if (b >= m.B) return;
    if (mask && mask[b] == 0) return;
    m.phase[b] = FRP_MISSION_IDLE; m.leg[b] = -1; m.tries[b] = 0;
    m.t_mark[b] = 0.0;
    m.issued[b] = 0; m.reached[b] = 0; m.dropped[b] = 0; m.abandoned[b] = 0; m.blocked[b] = 0;
    m.leg_time_sum[b] = 0.0; m.leg_time_max[b] = 0.0;
    m.goal[(size_t)b * 3] = 0.0; m.goal[(size_t)b * 3 + 1] = 0.0; m.goal[(size_t)b * 3 + 2] = 0.0;
    m.fresh[b] = 0;
}

// the arrays every call needs (host)
inline bool arrays_ok(const frp_nmpc_mission *m)
{
    return m && m->B >= 1 && m->phase && m->leg && m->tries && m->t_mark && m->issued && m->reached && m->dropped && m->abandoned && m->blocked &&
           m->leg_time_sum && m->leg_time_max && m->goal && m->fresh;
}

// the argument rules of a step's frp_nmpc_mission (host)
inline int check(const frp_nmpc_mission *m)
{
    if (!arrays_ok(m)) return FRP_ERR_ARG;
    if (!non_negative(m->arrive_radius) || !non_negative(m->dwell) || !non_negative(m->leg_timeout)) return FRP_ERR_ARG;
    if ((m->route != nullptr) == (m->R != 0)) return FRP_ERR_ARG; // neither mode, or both
    if (m->route) return m->W >= 1 && m->route_len ? FRP_OK : FRP_ERR_ARG;
    if (m->W != 0 || m->route_len || m->R < 1 || m->R > FRP_MISSION_MAX_TRIES) return FRP_ERR_ARG;
    for (int i = 0; i < 4; i++)
        if (!finite_d(m->goal_box[i])) return FRP_ERR_ARG;
    if (!(m->goal_box[0] < m->goal_box[1]) || !(m->goal_box[2] < m->goal_box[3]) || !finite_d(m->z_goal)) return FRP_ERR_ARG;
    if (!non_negative(m->min_dist) || !non_negative(m->max_dist) || m->min_dist > m->max_dist) return FRP_ERR_ARG;
    return FRP_OK;
}

} // namespace mission
} // namespace frp

extern "C" {

int frp_nmpc_mission_step(const frp_nmpc_mission *ms, const frp_nmpc_fsm *fsm, const double *state, const double *clock, const frp_nmpc_occmap *map,
                          const frp_nmpc_occmap_body *body, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::mission;
    namespace om = frp::occmap;
    if (check(ms) != FRP_OK || !fsm || !state || !clock || fsm->B != ms->B || !fsm->have_odom || !fsm->have_target || !fsm->end_pt) return FRP_ERR_ARG;
    om::Geo g = {};
    om::Half hf = {};
    const bool with_map = map || body || workspace;
    if (with_map) {
        if (ms->route || !map || !body || !workspace) return FRP_ERR_ARG;
        if (!om::args_ok(map, workspace, workspace_bytes) || !om::half_extents(map, body, ms->inflate_ratio, &hf)) return FRP_ERR_ARG;
        g = om::geo(map);
    }
    if (!frp::fleet::device_ok()) return FRP_ERR_NO_DEVICE;
    In in;
    in.have_odom = fsm->have_odom; in.have_target = fsm->have_target; in.end_pt = fsm->end_pt; in.state = state; in.clock = clock;
    hipLaunchKernelGGL(step_kernel, dim3(((unsigned)ms->B + 3u) / 4u), dim3(256), 0, static_cast<hipStream_t>(stream), *ms, in, g, hf,
                       with_map ? static_cast<const uint32_t *>(workspace) : nullptr);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_mission_clock(long long *k, double t0, double period, double dt, int n, double *clock, int advance, void *stream)
{
    using namespace frp::mission;
    if (!k || !clock || n < 1 || n > 64 || !finite_d(t0) || !non_negative(period) || !non_negative(dt) || advance < 0) return FRP_ERR_ARG;
    if (!frp::fleet::device_ok()) return FRP_ERR_NO_DEVICE;
    hipLaunchKernelGGL(clock_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), k, t0, period, dt, n, clock, advance);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_mission_reset(const frp_nmpc_mission *ms, const int *mask, void *stream)
{
    using namespace frp::mission;
    if (!arrays_ok(ms)) return FRP_ERR_ARG;
    if (!frp::fleet::device_ok()) return FRP_ERR_NO_DEVICE;
    return frp::fleet::launch(reset_kernel, frp::fleet::blocks_for(ms->B), stream, *ms, mask);
}

} // extern "C"
