// What the translation units of frp_nmpc.h section (8) share (frp_occmap.hip, frp_occmap_fuse.hip): the map's geometry as the kernels take
// it, the reference's index arithmetic (posToIndex, occ_map.cpp:71-75), the finiteness test and the argument checks of every call.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "frp_nmpc.h"

namespace frp {
namespace occmap {

constexpr double ID_LIM = 1073741824.0; // 2^30: floored indices are clamped here before they become int

struct Geo {
    double origin[3], res, res_inv;
    int grid[3], wz;
    double thr;
};

__host__ __device__ inline double floored(double p, double origin, double res_inv) { return floor((p - origin) * res_inv); } // posToIndex, :71-75

__host__ __device__ inline int clamp_id(double f)
{
    if (!(f >= -ID_LIM)) f = -ID_LIM; // NaN as well
    if (f > ID_LIM) f = ID_LIM;
    return (int)f;
}

__host__ __device__ inline bool finite_all(const double *a, int n)
{
    for (int i = 0; i < n; i++)
        if (!(fabs(a[i]) <= DBL_MAX)) return false; // std::isfinite
    return true;
}

inline size_t plane_bytes(const frp_nmpc_occmap *m) { return (size_t)m->grid[0] * m->grid[1] * ((m->grid[2] + 31) / 32) * sizeof(uint32_t); }

inline bool valid(const frp_nmpc_occmap *m)
{
    if (!m || !m->log_odds || !m->occ || !(m->resolution > 0.0) || !std::isfinite(m->resolution)) return false;
    for (int k = 0; k < 3; k++) {
        if (!(m->map_size[k] > 0.0) || !std::isfinite(m->map_size[k]) || !std::isfinite(m->origin[k])) return false;
        const double n = std::ceil(m->map_size[k] / m->resolution); // grid_size_, :789
        if (!(n >= 1.0 && n <= 65536.0) || m->grid[k] != (int)n) return false;
    }
    if ((size_t)m->grid[0] * m->grid[1] * m->grid[2] >= ((size_t)1 << 30)) return false; // voxel and column counts are int
    return std::isfinite(m->clamp_min_log) && std::isfinite(m->clamp_max_log) && std::isfinite(m->min_occupancy_log);
}

inline bool args_ok(const frp_nmpc_occmap *m, const void *ws, size_t ws_bytes) { return valid(m) && ws && ws_bytes >= plane_bytes(m); }

inline bool device_ok()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

inline Geo geo(const frp_nmpc_occmap *m)
{
    Geo g;
    for (int k = 0; k < 3; k++) { g.origin[k] = m->origin[k]; g.grid[k] = m->grid[k]; }
    g.res = m->resolution; g.res_inv = 1 / m->resolution; // resolution_inv_, :787
    g.wz = (m->grid[2] + 31) / 32;
    g.thr = m->min_occupancy_log;
    return g;
}

inline unsigned blocks_for(size_t n, unsigned cap = 8192)
{
    const size_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

} // namespace occmap
} // namespace frp
