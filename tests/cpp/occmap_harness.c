/* The occupancy map and its consumers driven from plain C through the C-ABI only (HIP runtime for memory; no torch, no C++):
 *   reset -> insert cloud -> local view -> corridor (per-planner clouds) + A* (map's occ, local boxes)
 *   occmap_harness <in.bin> <out.bin>
 * in.bin : int32 B, N, K, NP, P, allocate_num;  doubles origin[3], map_size[3], resolution, local_radius[3];  floats points[NP][3];
 *          doubles centre[B][3], ref_pos[B][N][3], ref_yaw[B][N], ellipsoid[B][N][9], start[B][3], end[B][3]
 * out.bin: doubles cloud[B][P][3], kino_path[B][K][3];  int32 local_box[B][6], cloud_count[B], poly_index[B][N], poly_nfaces[B][N],
 *          status[B], kino_size[B] */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "frp_nmpc.h"

#define CK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define FK(x) do { int rc_ = (x); if (rc_ != FRP_OK) { fprintf(stderr, "frp error %d at %s:%d\n", rc_, __FILE__, __LINE__); return 3; } } while (0)

static void *rd(FILE *f, size_t bytes)
{
    void *p = malloc(bytes ? bytes : 8);
    if (bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short read\n"); exit(4); }
    return p;
}
static void *up(const void *h, size_t bytes)
{
    void *d = NULL;
    if (hipMalloc(&d, bytes ? bytes : 8) != hipSuccess) exit(5);
    if (hipMemset(d, 0, bytes ? bytes : 8) != hipSuccess) exit(5);
    if (h && bytes && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) exit(5);
    return d;
}
static void *down(const void *d, size_t bytes)
{
    void *h = malloc(bytes ? bytes : 8);
    if (bytes && hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) exit(6);
    return h;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 1;
    if (FRP_NMPC_ABI_CHECK() != FRP_OK) return 7;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int *hdr = (int *)rd(f, 6 * sizeof(int));
    const int B = hdr[0], N = hdr[1], K = hdr[2], NP = hdr[3], P = hdr[4], alloc = hdr[5], F = 64;
    double *geo = (double *)rd(f, 10 * sizeof(double));
    float *pts = (float *)rd(f, sizeof(float) * 3 * (size_t)NP);
    double *centre = (double *)rd(f, sizeof(double) * 3 * B), *ref = (double *)rd(f, sizeof(double) * 3 * (size_t)B * N);
    double *yaw = (double *)rd(f, sizeof(double) * (size_t)B * N), *E = (double *)rd(f, sizeof(double) * 9 * (size_t)B * N);
    double *start = (double *)rd(f, sizeof(double) * 3 * B), *end = (double *)rd(f, sizeof(double) * 3 * B);
    fclose(f);
    hipStream_t st;
    CK(hipStreamCreate(&st));

    /* the map */
    frp_nmpc_occmap map = {.resolution = geo[6], .clamp_min_log = 0.12, .clamp_max_log = 0.97, .min_occupancy_log = 0.80};
    size_t voxels = 1;
    for (int i = 0; i < 3; i++) {
        map.origin[i] = geo[i]; map.map_size[i] = geo[3 + i]; map.local_radius[i] = geo[7 + i];
        map.grid[i] = (int)ceil(map.map_size[i] / map.resolution);
        voxels *= (size_t)map.grid[i];
    }
    map.log_odds = (double *)up(NULL, sizeof(double) * voxels);
    map.occ = (unsigned char *)up(NULL, voxels);
    const size_t mwb = frp_nmpc_occmap_workspace_bytes(&map);
    if (!mwb) return 8;
    void *d_mws = up(NULL, mwb);
    float *d_pts = (float *)up(pts, sizeof(float) * 3 * (size_t)NP);
    FK(frp_nmpc_occmap_reset(&map, d_mws, mwb, st));
    FK(frp_nmpc_occmap_insert_cloud(&map, d_pts, NP, d_mws, mwb, st));

    /* the views of B planners */
    double *d_centre = (double *)up(centre, sizeof(double) * 3 * B);
    int *d_box = (int *)up(NULL, sizeof(int) * 6 * B), *d_cnt = (int *)up(NULL, sizeof(int) * B);
    double *d_cloud = (double *)up(NULL, sizeof(double) * 3 * (size_t)B * P);
    frp_nmpc_occmap_view view = {.B = B, .centre = d_centre, .P = P, .local_box = d_box, .cloud = d_cloud, .cloud_count = d_cnt};
    FK(frp_nmpc_occmap_local_view(&map, &view, d_mws, mwb, st));

    /* corridor from the per-planner clouds */
    double *d_ref = (double *)up(ref, sizeof(double) * 3 * (size_t)B * N), *d_yaw = (double *)up(yaw, sizeof(double) * (size_t)B * N);
    double *d_E = (double *)up(E, sizeof(double) * 9 * (size_t)B * N);
    double *d_A = (double *)up(NULL, sizeof(double) * (size_t)B * N * F * 3), *d_b = (double *)up(NULL, sizeof(double) * (size_t)B * N * F);
    int *d_nf = (int *)up(NULL, sizeof(int) * (size_t)B * N), *d_pi = (int *)up(NULL, sizeof(int) * (size_t)B * N);
    frp_nmpc_corridor cr = {.B = B, .N = N, .F = F, .P = P, .cloud = d_cloud, .cloud_per_planner = 1, .cloud_count = d_cnt, .ref_pos = d_ref,
                            .ref_yaw = d_yaw, .ellipsoid = d_E, .bbox = {2.0, 2.0, 1.0}, .seed_len = 0.1, .inflation = 1.1, .offset_x = 0.0,
                            .poly_A = d_A, .poly_b = d_b, .poly_nfaces = d_nf, .poly_index = d_pi};
    FK(frp_nmpc_corridor_batch(&cr, st));

    /* A* on the map's byte grid inside every planner's local box */
    double *d_start = (double *)up(start, sizeof(double) * 3 * B), *d_end = (double *)up(end, sizeof(double) * 3 * B);
    double *d_zero = (double *)up(NULL, sizeof(double) * 3 * B);
    double *d_path = (double *)up(NULL, sizeof(double) * 3 * (size_t)B * K);
    int *d_ks = (int *)up(NULL, sizeof(int) * B), *d_status = (int *)up(NULL, sizeof(int) * B);
    frp_nmpc_astar as = {.B = B, .occ = map.occ, .resolution = map.resolution, .local_box = d_box, .ego_r = 0.27, .ego_h = 0.0425,
                         .max_tau = 0.5, .init_max_tau = 0.5, .max_vel = 2.0, .max_acc = 3.0, .w_time = 10.0, .horizon = 7.5, .lambda_heu = 5.0,
                         .tie_breaker = 1.0 + 1.0 / 10000, .allocate_num = alloc, .check_num = 15, .start_pt = d_start, .start_vel = d_zero,
                         .start_acc = d_zero, .end_pt = d_end, .end_vel = d_zero, .external_acc = d_zero, .init_search = 1, .Ts = 0.05, .K = K,
                         .kino_path = d_path, .kino_size = d_ks, .status = d_status};
    for (int i = 0; i < 3; i++) { as.grid[i] = map.grid[i]; as.origin[i] = map.origin[i]; as.map_size[i] = map.map_size[i]; }
    const size_t awb = frp_nmpc_astar_workspace_bytes(&as);
    void *d_aws = up(NULL, awb);
    FK(frp_nmpc_astar_batch(&as, d_aws, awb, st));
    CK(hipStreamSynchronize(st));

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 1;
    fwrite(down(d_cloud, sizeof(double) * 3 * (size_t)B * P), sizeof(double), 3 * (size_t)B * P, o);
    fwrite(down(d_path, sizeof(double) * 3 * (size_t)B * K), sizeof(double), 3 * (size_t)B * K, o);
    fwrite(down(d_box, sizeof(int) * 6 * B), sizeof(int), 6 * B, o);
    fwrite(down(d_cnt, sizeof(int) * B), sizeof(int), B, o);
    fwrite(down(d_pi, sizeof(int) * (size_t)B * N), sizeof(int), (size_t)B * N, o);
    fwrite(down(d_nf, sizeof(int) * (size_t)B * N), sizeof(int), (size_t)B * N, o);
    fwrite(down(d_status, sizeof(int) * B), sizeof(int), B, o);
    fwrite(down(d_ks, sizeof(int) * B), sizeof(int), B, o);
    fclose(o);
    return 0;
}
