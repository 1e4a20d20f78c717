// What the ray walks of the device occupancy map share: the bound on a ray's steps (ray-cast fusion, frp_occmap_fuse.hpp, and the two
// renderers, frp_occmap_render.hip and frp_occmap_render_scan.hip) and the renderers' choice of the next axis.  The renderers' slab walk
// itself -- ray set-up, plane reader with its held word, stepping loop -- is still written out in each render kernel: moved into
// functions here (three forms were tried) it compiles to other code, 2 - 3.5 % slower on an MI355X
// (profiles/occmap_sensor_refactor_identity.txt, profiles/occmap_sensor_refactor_bench.json), so the kernels keep their text.
#pragma once
#include "frp_occmap.hpp"

namespace frp {
namespace occmap {

constexpr int MAX_STEPS = 4096;

// The cells a ray of max_range can cross, with slack: the bound of every walk's loop.  false: more than MAX_STEPS, the call is refused.
inline bool step_bound(double max_range, double resolution, double *nb)
{
    *nb = 3.0 * (std::ceil(max_range / resolution) + 2.0);
    return *nb <= (double)MAX_STEPS;
}

namespace raywalk {

// the axis of the smallest crossing: the comparison tree of RayCaster::step (raycast.cpp:336-363)
__device__ inline int next_axis(const double *s_next)
{
    if (s_next[0] < s_next[1]) return s_next[0] < s_next[2] ? 0 : 2;
    return s_next[1] < s_next[2] ? 1 : 2;
}

} // namespace raywalk
} // namespace occmap
} // namespace frp
