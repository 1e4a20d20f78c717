// frp_copy_pool.hpp -- the host-buffer batch's staging copies (frp_host_batch.hip).  Plain C++17, no HIP: tests/cpp/copy_pool_harness.cpp
// drives it on its own under the thread and address sanitizers.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace frp::capi {
// A few persistent worker threads for the staging copies (user buffer <-> pinned block): one thread moves ~10-15 GB/s, the PCIe
// link 50; without them the host copy is the bottleneck of the whole path.
class CopyPool {
public:
    explicit CopyPool(int n) { for (int i = 0; i < n; i++) workers_.emplace_back([this] { run(); }); }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> l(m_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    void copy(void *dst, const void *src, size_t bytes)
    {
        const size_t parts = workers_.size() + 1, slice = ((bytes + parts - 1) / parts + 4095) / 4096 * 4096;
        if (bytes < (1u << 20) || workers_.empty()) { std::memcpy(dst, src, bytes); return; }
        size_t off = slice; // the caller's thread takes the first slice
        int queued = 0;
        {
            std::lock_guard<std::mutex> l(m_);
            for (; off < bytes; off += slice) { jobs_.push_back({static_cast<char *>(dst) + off, static_cast<const char *>(src) + off, std::min(slice, bytes - off), 0, 0, 0, 0, 0, 0}); queued++; }
            pending_ += queued;
        }
        cv_.notify_all();
        std::memcpy(dst, src, std::min(slice, bytes));
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return pending_ == 0; });
    }
    // `rows` parameter rows [10 | A (M x 3) | b (M)] -> [10 | A (MF x 3) | b (MF)]: the live corridor rows only (two segments per row)
    void pack_rows(double *dst, const double *src, size_t rows, int M, int MF)
    {
        const size_t parts = workers_.size() + 1, slice = (rows + parts - 1) / parts;
        Job proto{nullptr, nullptr, 0, 0, (10 + 3 * (size_t)MF) * 8, (size_t)MF * 8, (10 + 4 * (size_t)M) * 8, (10 + 4 * (size_t)MF) * 8, (10 + 3 * (size_t)M) * 8};
        auto make = [&](size_t r0, size_t n) { Job j = proto; j.d = reinterpret_cast<char *>(dst) + r0 * j.d_row; j.s = reinterpret_cast<const char *>(src) + r0 * j.s_row; j.rows = n; return j; };
        if (rows < 4096 || workers_.empty()) { run_job(make(0, rows)); return; }
        int queued = 0;
        {
            std::lock_guard<std::mutex> l(m_);
            for (size_t r0 = slice; r0 < rows; r0 += slice) { jobs_.push_back(make(r0, std::min(slice, rows - r0))); queued++; }
            pending_ += queued;
        }
        cv_.notify_all();
        run_job(make(0, std::min(slice, rows)));
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return pending_ == 0; });
    }
private:
    struct Job { char *d; const char *s; size_t n; size_t rows, a_bytes, b_bytes, s_row, d_row, s_boff; }; // rows == 0: one plain copy of n bytes
    static void run_job(const Job &j)
    {
        if (j.rows == 0) { std::memcpy(j.d, j.s, j.n); return; }
        // (rows of a few hundred bytes: plain loops the compiler vectorises, not two library calls per row)
        const size_t na = j.a_bytes / sizeof(double), nb = j.b_bytes / sizeof(double), so = j.s_boff / sizeof(double);
        for (size_t r = 0; r < j.rows; r++) {
            const double *sp = reinterpret_cast<const double *>(j.s + r * j.s_row);
            double *dp = reinterpret_cast<double *>(j.d + r * j.d_row);
            for (size_t i = 0; i < na; i++) dp[i] = sp[i];
            for (size_t i = 0; i < nb; i++) dp[na + i] = sp[so + i];
        }
    }
    void run()
    {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [this] { return stop_ || !jobs_.empty(); });
                if (stop_ && jobs_.empty()) return;
                j = jobs_.back(); jobs_.pop_back();
            }
            run_job(j);
            { std::lock_guard<std::mutex> l(m_); if (--pending_ == 0) done_.notify_all(); }
        }
    }
    std::vector<std::thread> workers_;
    std::vector<Job> jobs_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    int pending_ = 0;
    bool stop_ = false;
};
inline CopyPool &copy_pool()
{
    static CopyPool pool([] { const unsigned hc = std::thread::hardware_concurrency(); return (int)std::min(7u, hc > 2 ? hc / 2 - 1 : 0u); }());
    return pool;
}
} // namespace frp::capi
