// frp_fleet.hpp -- what the translation units of the fleet layer share (frp_nmpc.h sections 9-15: frp_command.hip, frp_outcome.hip,
// frp_fsm.hip, frp_vehicle.hip, frp_estimator.hip, frp_flight_record.hip, frp_disturbance.hip and frp_disturbance.hpp).
//
//   * Host part: what an entry point does around its own argument rules -- the device test, the finiteness predicates, the workgroup
//     width with its block count, and the launch.  Every entry point keeps the order FRP_ERR_ARG, FRP_ERR_NO_DEVICE, the B == 0 shortcut
//     where it has one, the launch.
//   * Device part: the maths more than one unit states -- Eigen's scalar quaternion product and toRotationMatrix, and the sampling of a
//     plan row at a time.  Every function is written one rounding per operation: no contraction here, as in the units (the build passes
//     -ffp-contract=off to each of them as well), so a unit's device code does not depend on whether it states a helper itself or takes
//     it from here (profiles/fleet_header_identity.txt).
//   * Kernels stay in their units: nothing here is a kernel, and nothing here stores to memory except through a caller's pointer.
//   * The occupancy map's units have a header of their own, frp_occmap.hpp, with its own device_ok(): it is not this one's business.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"

#pragma clang fp contract(off)

namespace frp {
namespace fleet {

// ---- host: around an entry point's own rules ----

constexpr int THREADS = 256; // a workgroup of every kernel of the layer
constexpr int ROW = 17;      // doubles in a plan row (layout.NZ)

inline bool device_ok()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// The finiteness tests, on comparisons alone: a NaN fails every comparison, so it fails each of them at its first test.
__host__ __device__ inline bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }   // finite
__host__ __device__ inline bool positive(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }      // finite and > 0
__host__ __device__ inline bool non_negative(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; } // finite and >= 0

// workgroups of THREADS for B items
inline unsigned blocks_for(long long B) { return (unsigned)((B + THREADS - 1) / THREADS); }

// `blocks` workgroups of THREADS of `kernel` on `stream`: FRP_OK when the launch was accepted
template <typename... P, typename... A>
inline int launch(void (*kernel)(P...), unsigned blocks, void *stream, const A &...args)
{
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream), args...);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

// ---- device: the maths more than one unit states ----

struct Quat {
    double w, x, y, z;
};

// a * b (Eigen Geometry/Quaternion.h, the scalar quat_product)
__device__ inline Quat qmul(const Quat &a, const Quat &b)
{
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}

// Quaternion::toRotationMatrix, row-major
__device__ inline void rotation(const Quat &q, double R[9])
{
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// Matrix3d(q) * (0, 0, thrust) (nmpc_solver.cpp:926-927, :176-178): the third column of rotation(q) times the thrust -- the products of the
// other two columns with the zeros of the body thrust add nothing for finite angles
__device__ inline void thrust_column(const Quat &q, double thrust, double *out)
{
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, txx = tx * q.x, txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y;
    out[0] = (txz + twy) * thrust;
    out[1] = (tyz - twx) * thrust;
    out[2] = (1.0 - (txx + tyy)) * thrust;
}

// Is t inside the plan (nmpc_solver.cpp:907-909, :164-167), on the doubles: for t >= 0 the truncation is a floor and
// floor(q) < N - 1 <=> q < N - 1; a NaN fails both comparisons, a quotient beyond int the second
__device__ inline bool in_plan(double t, double Ts, int N) { return t >= 0.0 && t / Ts < (double)(N - 1); }

// A plan sampled at a time t that is in_plan (mpcq, :907-911, :164-171): the stage, the fraction of it that has passed, and
// q <- row[i] + w * (row[i + 1] - row[i]) -- the host's operations, one rounding each, an IEEE division, ocml's exact fmod.
// `first`: the plan's first row in `plan` (planner * N).  Slots 4-7 (the previous input) are not sampled: zeros.
// The stage and the fraction are arguments, not computed inside plan_row from (t, Ts): with that shape, and with the row's address
// formed at the call site, frp_fsm.hip's exec_begin_kernel came out with other bytes than it had with the sampling written out.
__device__ inline int plan_stage(double t, double Ts) { return (int)(t / Ts); }
__device__ inline double plan_fraction(double t, double Ts) { return fmod(t, Ts) / Ts; }
__device__ inline void plan_row(const double *plan, size_t first, int idx, double w, double q[ROW])
{
    const double *r0 = plan + (first + idx) * ROW, *r1 = r0 + ROW;
#pragma unroll
    for (int j = 0; j < ROW; j++) q[j] = (j >= 4 && j < 8) ? 0.0 : r0[j] + w * (r1[j] - r0[j]);
}

} // namespace fleet
} // namespace frp
