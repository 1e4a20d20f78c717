// Host check of the staging copies of the host-buffer batch (csrc/frp_copy_pool.hpp): CopyPool::copy and CopyPool::pack_rows against plain
// loops, on both sides of the thresholds at which the pool's workers take part (1 MiB, 4096 rows), at sizes that are no multiple of a slice,
// from two caller threads one after the other.  Built with the thread and the address sanitizer by tests/test_copy_pool_cpu.py; the pool's
// size follows hardware_concurrency(), so on a small machine the same calls run on the caller's thread alone.
//   copy_pool_harness        prints "ok <calls>" and returns 0, or names the first mismatch and returns 1
#include <cstdio>
#include <thread>
#include <vector>
#include "../../forces_resilient_planner_amd/csrc/frp_copy_pool.hpp"

static int check_copy(size_t bytes)
{
    std::vector<unsigned char> src(bytes + 64), dst(bytes + 64, 0xEE);
    for (size_t i = 0; i < src.size(); i++) src[i] = (unsigned char)(i * 131 + (i >> 8));
    frp::capi::copy_pool().copy(dst.data(), src.data(), bytes);
    for (size_t i = 0; i < dst.size(); i++)
        if (dst[i] != (i < bytes ? src[i] : 0xEE)) { fprintf(stderr, "copy(%zu): byte %zu\n", bytes, i); return 1; }
    return 0;
}

static int check_pack(size_t rows, int M, int MF)
{
    const size_t sr = 10 + 4 * (size_t)M, dr = 10 + 4 * (size_t)MF;
    std::vector<double> src(rows * sr), dst(rows * dr + 8, -7.0);
    for (size_t i = 0; i < src.size(); i++) src[i] = (double)i + 0.25;
    frp::capi::copy_pool().pack_rows(dst.data(), src.data(), rows, M, MF);
    for (size_t r = 0; r < rows; r++)
        for (size_t e = 0; e < dr; e++) { // [10 | A (MF x 3)] from the row's head, [b (MF)] from behind the M rows of A
            const size_t from = e < 10 + 3 * (size_t)MF ? e : e - (10 + 3 * (size_t)MF) + 10 + 3 * (size_t)M;
            if (dst[r * dr + e] != src[r * sr + from]) { fprintf(stderr, "pack_rows(%zu, %d, %d): row %zu element %zu\n", rows, M, MF, r, e); return 1; }
        }
    for (size_t i = rows * dr; i < dst.size(); i++)
        if (dst[i] != -7.0) { fprintf(stderr, "pack_rows(%zu, %d, %d): wrote past the end\n", rows, M, MF); return 1; }
    return 0;
}

int main()
{
    const size_t bytes[] = {0, 8, (1u << 20) - 8, 1u << 20, (1u << 20) + 8, (3u << 20) + 4104};
    const size_t rows[] = {1, 4095, 4096, 4097, 12289};
    const int shapes[][2] = {{30, 6}, {30, 0}, {7, 7}};
    int bad = 0, calls = 0;
    for (int caller = 0; caller < 2; caller++) {
        std::thread t([&] {
            for (size_t b : bytes) { bad += check_copy(b); calls++; }
            for (size_t r : rows)
                for (auto &s : shapes) { bad += check_pack(r, s[0], s[1]); calls++; }
        });
        t.join();
    }
    if (bad) return 1;
    printf("ok %d\n", calls);
    return 0;
}
