// frp_occmap_check.hpp -- what the units that probe the map's bit plane with a whole wavefront share (frp_occmap_check.hip, section 8's
// safety checks, and frp_mission.hip, section 17's goal draws): OccMap::checkPosSurround (occ_grid/src/occ_map.cpp:625-643) by one
// wavefront, the three wave reductions it takes, and the half extents of the inflated body.  The text is frp_occmap_check.hip's as it
// was, moved (profiles/mission_check_identity.txt: that unit's device code did not change); the comment at the head of that file says
// how the probe works.  Both units are built with -ffp-contract=off: pos + i * resolution is a product and a sum.
#pragma once
#include "frp_occmap.hpp"

namespace frp {
namespace occmap {

constexpr int CHECK_MAX_HALF = 31; // 2 * 31 + 1 = 63 offsets per axis: one lane each

struct Half {
    int h[3];
};

__device__ inline int wave_min(int v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ inline int wave_max(int v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline uint32_t wave_or(uint32_t v)
{
    for (int d = 32; d > 0; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// checkPosSurround(p, .) (:625-643) by one whole wavefront; the result is the same in every lane.  bx: the planner's row of
// local_box or null.  Every lane of the wavefront must call it (shuffles and votes).
__device__ inline bool surround_free(const Geo &g, const Half &hf, double px, double py, double pz, const int *bx, const uint32_t *plane, int lane)
{
    const double p[3] = {px, py, pz};
    int id[3]; // this lane's voxel index per axis; -1: no probe survives (lane beyond the extent, or outside the local box)
    bool outside = false;
    // (selects, no nested branches: the three axes are the same straight-line code)
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int lo = bx ? bx[a] : 0, hi = bx ? bx[3 + a] : 0x7fffffff; // isInLocalMap (:56), INCLUSIVE on both sides
        const bool active = lane <= 2 * hf.h[a];
        const double f = floored(p[a] + (double)(lane - hf.h[a]) * g.res, g.origin[a], g.res_inv); // :635, posToIndex :71-75
        const bool in_map = f >= 0.0 && f <= (double)(g.grid[a] - 1);                              // isInMap (:66-69); a NaN fails both comparisons
        const int v = in_map ? (int)f : -1;
        outside = outside || (active && !in_map);
        id[a] = active && in_map && v >= lo && v <= hi ? v : -1;
    }
    if (__any(outside)) return false; // state -1 (:99-100) for every probe that shares this index
    const int zw = id[2] >> 5; // (-1 stays -1)
    const int whi = wave_max(zw);
    if (whi < 0) return true; // the local box hides every z
    const int wlo = wave_min(id[2] >= 0 ? zw : 0x7fffffff);
    const int ny = 2 * hf.h[1] + 1, ncols = (2 * hf.h[0] + 1) * ny;
    for (int w = wlo; w <= whi; w++) { // one word for most bodies, at most three for 63 offsets
        const uint32_t mask = wave_or(id[2] >= 0 && zw == w ? 1u << (id[2] & 31) : 0u);
        if (!mask) continue;
        for (int c0 = 0; c0 < ncols; c0 += 64) {
            const int c = c0 + lane;
            const bool have = c < ncols;
            const int x = __shfl(id[0], have ? c / ny : 0, 64), y = __shfl(id[1], have ? c % ny : 0, 64);
            bool hit = false;
            if (have && x >= 0 && y >= 0) hit = (plane[((size_t)x * g.grid[1] + y) * g.wz + w] & mask) != 0; // :105 on the bit plane
            if (__any(hit)) return false;
        }
    }
    return true;
}

// x_size, y_size, z_size of :627-629: ceil(ego * inflate_ratio / resolution_), in that order
static bool half_extents(const frp_nmpc_occmap *m, const frp_nmpc_occmap_body *body, double inflate_ratio, Half *hf)
{
    if (!body) return false;
    const double e[3] = {body->ego_r, body->ego_r, body->ego_h};
    for (int k = 0; k < 3; k++) {
        const double c = std::ceil(e[k] * inflate_ratio / m->resolution);
        if (!(c >= 0.0 && c <= (double)CHECK_MAX_HALF)) return false; // a NaN as well
        hf->h[k] = (int)c;
    }
    return true;
}

} // namespace occmap
} // namespace frp
