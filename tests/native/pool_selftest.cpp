// pool_selftest.cpp — aqc_pool.hpp's lane policy (test infrastructure; built and run by tests/test_gz_codec.py):
//   * front jobs overtake queued background jobs: with every worker busy and both lanes full, all front jobs are started
//     before any further background job is;
//   * help_front() runs a queued front job on the calling thread and reports an empty lane;
//   * parallel_for still completes with the pool saturated by background jobs;
//   * help_front() never runs the helper closure of another thread's parallel_for.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_pool.hpp"

int main() {
    using namespace std::chrono;
    int failures = 0;
    // A job takes its rank in its body, i.e. after the worker has dequeued it and let go of the pool's lock.  With one worker the
    // ranks ARE the dequeue order, and the rule is checked to the letter: every front job before any queued background job.  With
    // four, a worker that has taken one of the last front jobs can lose the CPU before it ranks, while another finds the front
    // lane empty, rightly takes a background job and ranks first: when the first background job ranks, each of the other
    // workers - 1 threads may hold one front job in that window, and no more than that may rank after it.  (A pool that serves
    // the lanes in turn puts some 28 of the 32 there.)
    for (int workers : {1, 4}) {
        aqc_host::Pool pool(workers);
        std::atomic<int> gate{0}, order{0}, bg_started{0}, front_done{0};
        std::vector<int> front_rank(32, -1), bg_rank(16, -1);
        // background jobs occupy the workers until the gate opens
        for (int i = 0; i < workers; ++i)
            pool.submit([&] { bg_started++; while (!gate.load()) std::this_thread::sleep_for(microseconds(50)); }, true);
        while (bg_started.load() < workers) std::this_thread::sleep_for(microseconds(50));
        // now both lanes fill up while nobody can take anything
        for (int i = 0; i < 16; ++i) pool.submit([&, i] { bg_rank[i] = order++; std::this_thread::sleep_for(microseconds(200)); }, true);
        for (int i = 0; i < 32; ++i) pool.submit([&, i] { front_rank[i] = order++; front_done++; }, false);
        gate = 1;
        const auto t0 = steady_clock::now();
        while (order.load() < 48 && steady_clock::now() - t0 < seconds(20)) std::this_thread::sleep_for(microseconds(100));
        int worst_front = -1, first_bg = 1 << 30, late_front = 0;
        for (int r : front_rank) worst_front = r > worst_front ? r : worst_front;
        for (int r : bg_rank) first_bg = r < first_bg ? r : first_bg;
        for (int r : front_rank) late_front += r > first_bg;
        const bool ok = order.load() == 48 && worst_front >= 0 && first_bg >= 0 && late_front <= workers - 1;
        printf("front lane first, %d worker(s): last front job ranked %d, first queued background job %d, %d front job(s) ranked after it (at most %d)  %s\n",
               workers, worst_front, first_bg, late_front, workers - 1, ok ? "ok" : "FAIL");
        if (!ok) ++failures;
    }
    {
        aqc_host::Pool pool(2);
        std::atomic<int> gate{0}, started{0}, ran{0};
        for (int i = 0; i < 2; ++i) pool.submit([&] { started++; while (!gate.load()) std::this_thread::sleep_for(microseconds(50)); }, true);
        while (started.load() < 2) std::this_thread::sleep_for(microseconds(50));
        const std::thread::id me = std::this_thread::get_id();
        std::atomic<int> on_caller{0};
        for (int i = 0; i < 5; ++i) pool.submit([&] { ran++; if (std::this_thread::get_id() == me) on_caller++; }, false);
        int helped = 0;
        while (pool.help_front()) ++helped;
        const bool ok = helped == 5 && ran.load() == 5 && on_caller.load() == 5 && !pool.help_front();
        printf("help_front: %d jobs run by the caller while the workers were busy  %s\n", helped, ok ? "ok" : "FAIL");
        if (!ok) ++failures;
        // parallel_for with the workers still stuck: the caller does the work
        std::atomic<long> sum{0};
        pool.parallel_for(100, [&](size_t i) { sum += (long)i; });
        const bool ok2 = sum.load() == 4950;
        printf("parallel_for under saturation: sum %ld  %s\n", sum.load(), ok2 ? "ok" : "FAIL");
        if (!ok2) ++failures;
        gate = 1;
    }
    {
        // help_front never takes the helper closure of somebody else's parallel_for (it would sit in that batch until it is done):
        // with the workers stuck, a thread in a long parallel_for has its helpers queued; the main thread's help_front must find only
        // the job that was SUBMITTED — and report an empty lane afterwards although the helpers are still there.
        aqc_host::Pool pool(2);
        std::atomic<int> gate{0}, started{0}, batch_gate{0}, in_batch{0}, submitted_ran{0};
        for (int i = 0; i < 2; ++i) pool.submit([&] { started++; while (!gate.load()) std::this_thread::sleep_for(microseconds(50)); }, true);
        while (started.load() < 2) std::this_thread::sleep_for(microseconds(50));
        const std::thread::id me = std::this_thread::get_id();
        std::atomic<int> batch_on_me{0};
        std::thread other([&] {
            pool.parallel_for(8, [&](size_t) {
                in_batch++;
                if (std::this_thread::get_id() == me) batch_on_me++;
                while (!batch_gate.load()) std::this_thread::sleep_for(microseconds(50));
            });
        });
        while (in_batch.load() < 1) std::this_thread::sleep_for(microseconds(50));       // (its helpers are queued, it works on index 0)
        pool.submit([&] { submitted_ran++; }, false);
        int helped = 0;
        while (pool.help_front()) ++helped;
        const bool ok = helped == 1 && submitted_ran.load() == 1 && batch_on_me.load() == 0;
        printf("help_front leaves parallel_for helpers alone: helped %d, batch indices run by the helper %d  %s\n", helped, batch_on_me.load(), ok ? "ok" : "FAIL");
        if (!ok) ++failures;
        batch_gate = 1;
        gate = 1;
        other.join();
    }
    if (failures) { printf("%d pool checks FAILED\n", failures); return 1; }
    printf("all pool checks passed\n");
    return 0;
}
