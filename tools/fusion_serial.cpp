// A single-thread C++ PORT of the serial depth-frame fusion -- NOT the reference: the reference's OccMap needs ROS, Eigen and OpenCV
// and is not compiled here.  This program follows tests/occmap_fusion_oracle.py statement by statement (unfiltered projection, end-voxel
// dedup, backwards ray cast with the traverse break, batch update) with the reference's data layout: whole-map int arrays stamped with
// the frame number and a queue of touched voxels.  tools/fusion_bench.py builds it, feeds it a frame and records its host time next to
// the device's; it also counts what needs no device: rays cast, cells the serial scan processes, cells of the full paths, and the
// rounds the round-based form (raycast_relaxed, what frp_occmap_fuse.hip runs) needs to reach the serial stops.
//
//   c++ -O2 -std=c++17 -o fusion_serial tools/fusion_serial.cpp && ./fusion_serial frame.bin [reps=10]
// frame.bin: int32 rows, cols, margin, skip, grid[3], pad; double origin[3], resolution, K[9], T_wc[16], depth_scale, mindist,
// prob_hit_log, prob_miss_log, min_ray_length, max_ray_length, clamp_min_log, clamp_max_log; uint16 depth[rows][cols].
// Prints one JSON line.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Frame {
    int32_t rows, cols, margin, skip, grid[3], pad;
    double origin[3], res, K[9], T[16], depth_scale, mindist, hit_log, miss_log, min_len, max_len, cmin, cmax;
};

struct Map {
    Frame f;
    double res_inv;
    std::vector<double> log_odds;
    std::vector<int> all, hit, rayend, traverse, touched;
    int frame_no = 0;

    explicit Map(const Frame &fr) : f(fr), res_inv(1 / fr.res)
    {
        const size_t n = (size_t)f.grid[0] * f.grid[1] * f.grid[2];
        log_odds.assign(n, f.cmin);
        all.assign(n, 0); hit.assign(n, 0); rayend.assign(n, 0); traverse.assign(n, 0);
    }

    int index(const double *p) const // posToIndex + isInMap: the linear voxel index or -1
    {
        int id[3];
        for (int k = 0; k < 3; k++) {
            const double fl = std::floor((p[k] - f.origin[k]) * res_inv);
            if (!(fl >= 0.0 && fl <= (double)(f.grid[k] - 1))) return -1;
            id[k] = (int)fl;
        }
        return (id[0] * f.grid[1] + id[1]) * f.grid[2] + id[2];
    }

    int cache(const double *p, int occ) // setCacheOccupancy
    {
        const int v = index(p);
        if (v < 0) return -1;
        if (++all[v] == 1) touched.push_back(v);
        if (occ) hit[v]++;
        return v;
    }
};

static double rc_mod(double value, double modulus) { return std::fmod(std::fmod(value, modulus) + modulus, modulus); }

static double intbound(double s, double ds)
{
    if (ds < 0) { s = -s; ds = -ds; }
    s = rc_mod(s, 1.0);
    return (1 - s) / ds;
}

static int sgn(double d) { return d == 0.0 ? 0 : d < 0.0 ? -1 : 1; }

struct Caster {
    int x, y, z, ex, ey, ez, sx, sy, sz;
    double tmx, tmy, tmz, tdx, tdy, tdz;

    bool set_input(const double *s, const double *e)
    {
        x = (int)std::floor(s[0]); y = (int)std::floor(s[1]); z = (int)std::floor(s[2]);
        ex = (int)std::floor(e[0]); ey = (int)std::floor(e[1]); ez = (int)std::floor(e[2]);
        const double dx = ex - x, dy = ey - y, dz = ez - z;
        sx = sgn(dx); sy = sgn(dy); sz = sgn(dz);
        tmx = intbound(s[0], dx); tmy = intbound(s[1], dy); tmz = intbound(s[2], dz);
        tdx = sx / dx; tdy = sy / dy; tdz = sz / dz;
        return !(sx == 0 && sy == 0 && sz == 0);
    }
    bool at_end() const { return x == ex && y == ey && z == ez; }
    void advance()
    {
        if (tmx < tmy) {
            if (tmx < tmz) { x += sx; tmx += tdx; } else { z += sz; tmz += tdz; }
        } else {
            if (tmy < tmz) { y += sy; tmy += tdy; } else { z += sz; tmz += tdz; }
        }
    }
};

struct Ray { int seq; double p[3]; };

static void project(const Frame &f, const uint16_t *depth, std::vector<Ray> &pts)
{
    pts.clear();
    int seq = 0;
    for (int v = f.margin; v < f.rows - f.margin; v += f.skip)
        for (int u = f.margin; u < f.cols - f.margin; u += f.skip, seq++) {
            const double d = (double)depth[(size_t)v * f.cols + u] / f.depth_scale;
            if (d < f.mindist) continue;
            const double x = ((double)u - f.K[2]) * d / f.K[0], y = ((double)v - f.K[5]) * d / f.K[4], z = d;
            Ray r; r.seq = seq;
            for (int i = 0; i < 3; i++) r.p[i] = ((f.T[4 * i] * x + f.T[4 * i + 1] * y) + f.T[4 * i + 2] * z) + f.T[4 * i + 3];
            pts.push_back(r);
        }
}

// The head of the per-point loop: length test, clip, end voxel bookkeeping, dedup.  true: the point casts its ray (from pt, updated).
static bool ray_end(Map &m, double *pt, const double *t)
{
    const Frame &f = m.f;
    const double d[3] = {pt[0] - t[0], pt[1] - t[1], pt[2] - t[2]};
    const double length = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (length < f.min_len) return false;
    int occ = 1;
    if (length > f.max_len) {
        for (int i = 0; i < 3; i++) pt[i] = d[i] / length * f.max_len + t[i];
        occ = 0;
    }
    const int e = m.cache(pt, occ);
    if (e >= 0) {
        if (m.rayend[e] == m.frame_no) return false;
        m.rayend[e] = m.frame_no;
    }
    return true;
}

static void batch_update(Map &m)
{
    const Frame &f = m.f;
    for (int v : m.touched) {
        const double upd = m.hit[v] >= m.all[v] - m.hit[v] ? f.hit_log : f.miss_log;
        m.hit[v] = m.all[v] = 0;
        const double cur = m.log_odds[v];
        if ((upd >= 0 && cur >= f.cmax) || (upd <= 0 && cur <= f.cmin)) continue;
        m.log_odds[v] = std::min(std::max(cur + upd, f.cmin), f.cmax);
    }
    m.touched.clear();
}

struct Counts { long rays = 0, steps = 0; };

// One frame, serially.  stops (optional): cells processed per cast ray, in scan order.
static Counts serial_frame(Map &m, const uint16_t *depth, std::vector<Ray> &pts, int nb, std::vector<int> *stops)
{
    const Frame &f = m.f;
    const double t[3] = {f.T[3], f.T[7], f.T[11]};
    Counts c;
    project(f, depth, pts);
    if (pts.empty()) return c;
    m.frame_no++;
    for (Ray &r : pts) {
        if (!ray_end(m, r.p, t)) continue;
        c.rays++;
        const double s[3] = {r.p[0] / f.res, r.p[1] / f.res, r.p[2] / f.res}, e[3] = {t[0] / f.res, t[1] / f.res, t[2] / f.res};
        Caster rc;
        if (!rc.set_input(s, e) || rc.at_end()) continue;
        rc.advance(); // the ray start is skipped
        int n = 0;
        while (n < nb && !rc.at_end()) {
            const double p[3] = {(rc.x + 0.5) * f.res, (rc.y + 0.5) * f.res, (rc.z + 0.5) * f.res};
            rc.advance();
            n++;
            const int v = m.cache(p, 0);
            if (v >= 0) {
                if (m.traverse[v] == m.frame_no) break; // counted above, then the break
                m.traverse[v] = m.frame_no;
            }
        }
        c.steps += n;
        if (stops) stops->push_back(n);
    }
    batch_update(m);
    return c;
}

// The same frame by rounds (raycast_relaxed): full paths, then mark / stop rounds up to and including the first that changes
// nothing.  Returns the rounds; fills the full-path cell count and the final stops.
static int relaxed_rounds(const Frame &f, const uint16_t *depth, int nb, long *full_steps, std::vector<int> *stops)
{
    Map m(f);
    const double t[3] = {f.T[3], f.T[7], f.T[11]};
    std::vector<Ray> pts;
    project(f, depth, pts);
    m.frame_no++;
    std::vector<std::vector<int>> paths;
    for (Ray &r : pts) {
        if (!ray_end(m, r.p, t)) continue;
        const double s[3] = {r.p[0] / f.res, r.p[1] / f.res, r.p[2] / f.res}, e[3] = {t[0] / f.res, t[1] / f.res, t[2] / f.res};
        Caster rc;
        if (!rc.set_input(s, e) || rc.at_end()) continue;
        rc.advance();
        std::vector<int> path;
        while ((int)path.size() < nb && !rc.at_end()) {
            const double p[3] = {(rc.x + 0.5) * f.res, (rc.y + 0.5) * f.res, (rc.z + 0.5) * f.res};
            rc.advance();
            path.push_back(m.index(p));
        }
        paths.push_back(std::move(path));
    }
    *full_steps = 0;
    std::vector<int> count(paths.size());
    for (size_t i = 0; i < paths.size(); i++) { count[i] = (int)paths[i].size(); *full_steps += count[i]; }
    std::vector<int> mark(m.log_odds.size(), INT_MAX);
    int rounds = 0;
    for (bool changed = true; changed;) {
        rounds++;
        for (size_t i = 0; i < paths.size(); i++)
            for (int k = 0; k < count[i]; k++) {
                const int v = paths[i][k];
                if (v >= 0 && mark[v] > (int)i) mark[v] = (int)i;
            }
        changed = false;
        for (size_t i = 0; i < paths.size(); i++) {
            int c = (int)paths[i].size(), prev = -1;
            for (int k = 0; k < (int)paths[i].size(); k++) {
                const int v = paths[i][k];
                if (v < 0) continue;
                if (mark[v] < (int)i || v == prev) { c = k + 1; break; }
                prev = v;
            }
            if (c != count[i]) { count[i] = c; changed = true; }
        }
        for (const auto &p : paths)
            for (int v : p)
                if (v >= 0) mark[v] = INT_MAX;
    }
    *stops = count;
    return rounds;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s frame.bin [reps]\n", argv[0]); return 2; }
    const int reps = argc > 2 ? std::atoi(argv[2]) : 10;
    FILE *fp = std::fopen(argv[1], "rb");
    Frame f;
    if (!fp || std::fread(&f, sizeof f, 1, fp) != 1 || f.rows < 1 || f.cols < 1 || f.skip < 1 || f.margin < 0 || reps < 1) {
        std::fprintf(stderr, "cannot read the frame header of %s\n", argv[1]);
        return 2;
    }
    std::vector<uint16_t> depth((size_t)f.rows * f.cols);
    if (std::fread(depth.data(), 2, depth.size(), fp) != depth.size()) { std::fprintf(stderr, "short depth image\n"); return 2; }
    std::fclose(fp);
    const int nb = 3 * ((int)std::ceil(f.max_len / f.res) + 2);

    Map m(f);
    std::vector<Ray> pts;
    std::vector<int> serial_stops;
    const Counts c = serial_frame(m, depth.data(), pts, nb, &serial_stops); // also the warm-up
    std::vector<double> ms;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        const Counts again = serial_frame(m, depth.data(), pts, nb, nullptr);
        const auto t1 = std::chrono::steady_clock::now();
        if (again.rays != c.rays || again.steps != c.steps) { std::fprintf(stderr, "the frame is not repeatable\n"); return 1; }
        ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    long full = 0;
    std::vector<int> relaxed_stops;
    const int rounds = relaxed_rounds(f, depth.data(), nb, &full, &relaxed_stops);
    std::printf("{\"what\": \"single-thread C++ port of the serial scan, not the reference\", \"reps\": %d, \"host_ms_min\": %.4f, "
                "\"host_ms_median\": %.4f, \"host_ms_max\": %.4f, \"rays\": %ld, \"serial_steps\": %ld, \"full_path_steps\": %ld, "
                "\"rounds\": %d, \"relaxed_equals_serial\": %s}\n",
                reps, ms.front(), ms[ms.size() / 2], ms.back(), c.rays, c.steps, full, rounds,
                relaxed_stops == serial_stops ? "true" : "false");
    return relaxed_stops == serial_stops ? 0 : 1;
}
