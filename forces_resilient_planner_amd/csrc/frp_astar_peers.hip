// frp_astar_peers.hip -- frp_nmpc.h section (19): the kinodynamic A* on the map plus a planner's peer boxes.  The search is
// frp_astar.hip's text, compiled a second time with the overlay: a voxel is occupied where the map says so OR it lies in one of the
// planner's boxes, on every lookup route -- the staged LDS window (the boxes' z masks are OR-ed into the words as they are staged, so the
// cell-box fast path reads them with the map's bits), the packed map's own word outside the window, and the byte map of grid[2] > 64.
// Contributes frp_nmpc_astar_batch_peers and the kernels of frp::astar_peers; frp_nmpc_astar_batch and frp::astar stay frp_astar.hip's.
// Built with that unit's flags (-ffp-contract=off): the same arithmetic, the same bits.
#define FRP_ASTAR_PEERS
#include "frp_astar.hip"
