// aqc_pipe_prim.hpp — the small things every stage of the whole-input pipe uses: clocks, the bounded queue the threads hand
// work over with, and the reading of on / off environment knobs.  Part of aqc_pipe.cpp's translation unit (included there only).
#pragma once

#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <ctime>
#include <deque>
#include <mutex>

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
double thread_cpu_s() {
    timespec ts;
    return clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0 ? (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec : 0.0;
}
double process_cpu_s() {
    timespec ts;
    return clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &ts) == 0 ? (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec : 0.0;
}
uint64_t now_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class T>
class BQueue {
public:
    explicit BQueue(size_t cap = 0) : cap_(cap) {}
    bool push(T v) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_space_.wait(lk, [&] { return closed_ || cap_ == 0 || q_.size() < cap_; });
        if (closed_) return false;
        q_.push_back(std::move(v));
        cv_item_.notify_one();
        return true;
    }
    bool pop(T& out) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_item_.wait(lk, [&] { return closed_ || !q_.empty(); });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        cv_space_.notify_one();
        return true;
    }
    void close() {
        std::lock_guard<std::mutex> g(mu_);
        closed_ = true;
        cv_item_.notify_all();
        cv_space_.notify_all();
    }

private:
    size_t cap_;
    std::deque<T> q_;
    std::mutex mu_;
    std::condition_variable cv_item_, cv_space_;
    bool closed_ = false;
};

// an on / off knob of the environment: on unless its value starts with '0' (AQC_GZ_DEVICE=0, AQC_GZ_HBM=0, ...).  Read where a run
// starts or a source is opened, never kept across runs: the tests switch knobs between runs of one process.
inline bool env_on(const char* name) {
    const char* e = getenv(name);
    return !(e && e[0] == '0');
}

}  // namespace
