// keep_selftest.cpp — aqc_keep.hpp, the keeper of the device decoders (test infrastructure; built and run by tests/test_keep.py,
// plain and with -fsanitize=address,undefined):
//   * take() on an empty keeper gives null; give() then take() with an equal key returns that very object;
//   * take() with a key that differs in ONE field gives null — the device, and every field of aqcgz::OffloadOpts, the key of a
//     gunzip decoder (a field that operator== forgets fails here; a field that is added fails to compile until it is covered);
//   * the 17th give() returns the object to the caller and 16 stay;
//   * lend() twice with one key calls make() once and returns one pointer; take() never returns a lent object;
//   * eight threads doing take() / give() on four keys a thousand times each lose and duplicate nothing;
//   * nothing that is kept or lent is ever destroyed: an atexit handler registered before the keepers' first use — it runs after
//     every static destructor registered later — sees no destruction that the test did not do itself; and LeakSanitizer stays
//     silent, because what is kept is reachable through the plain pointers that hold the keepers.
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <utility>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_gz.hpp"
#include "../../afterqc_amd/csrc/aqc_keep.hpp"

namespace {

std::atomic<int> g_made{0}, g_destroyed{0};
int g_destroyed_by_test = 0;       // what main() destroyed itself, on purpose: all that may be gone at exit()

struct Payload {
    int id;
    std::atomic<int> users{0};
    explicit Payload(int i) : id(i) { g_made++; }
    ~Payload() { g_destroyed++; }
};

using GzKey = std::pair<int, aqcgz::OffloadOpts>;
using GzKeep = aqc::Keep<GzKey, Payload>;
using IntKeep = aqc::Keep<int, Payload>;
// held as the library holds its keepers: plain pointers with static storage, the objects on the heap
GzKeep* g_gz;
IntKeep* g_cap;
IntKeep* g_lend;
IntKeep* g_threads;

int failures = 0;
void check(bool ok, const char* what) {
    printf("%-100s %s\n", what, ok ? "ok" : "FAIL");
    if (!ok) ++failures;
}

void at_exit() {
    // (stdio may be gone by now: write(2), and _exit so that the status stands)
    if (g_destroyed.load() != g_destroyed_by_test) {
        const char msg[] = "FAIL: a kept payload was destroyed at exit\n";
        (void)!write(2, msg, sizeof(msg) - 1);
        _exit(3);
    }
    const char msg[] = "at exit: no kept payload was destroyed\n";
    (void)!write(1, msg, sizeof(msg) - 1);
}

}  // namespace

int main() {
    atexit(at_exit);
    setvbuf(stdout, nullptr, _IONBF, 0);
    g_gz = new GzKeep;
    g_cap = new IntKeep;
    g_lend = new IntKeep;
    g_threads = new IntKeep;

    // ---- one object, every field of its key ---------------------------------------------------------------------------------------
    {
        const aqcgz::OffloadOpts base = aqcgz::OffloadOpts{4u << 20, true, 6, 1, 512, true};
        auto [f_group, f_resident, f_ratio, f_tok, f_overlap, f_grow] = base;       // (six fields: a seventh does not compile here)
        (void)f_group; (void)f_resident; (void)f_ratio; (void)f_tok; (void)f_overlap; (void)f_grow;
        const GzKey key(0, base);
        check(!g_gz->take(key), "take() on an empty keeper gives null");
        Payload* p = new Payload(1);
        check(!g_gz->give(key, std::unique_ptr<Payload>(p)), "give() keeps the object");
        std::vector<std::pair<const char*, GzKey>> others;
        others.emplace_back("device", GzKey(1, base));
        aqcgz::OffloadOpts o = base; o.group_bytes = 8u << 20; others.emplace_back("group_bytes", GzKey(0, o));
        o = base; o.resident = false; others.emplace_back("resident", GzKey(0, o));
        o = base; o.ratio_cap = 12; others.emplace_back("ratio_cap", GzKey(0, o));
        o = base; o.tok_ratio = 6; others.emplace_back("tok_ratio", GzKey(0, o));
        o = base; o.overlap_tokens = 2048; others.emplace_back("overlap_tokens", GzKey(0, o));
        o = base; o.grow = false; others.emplace_back("grow", GzKey(0, o));
        for (auto& e : others) {
            char what[128];
            snprintf(what, sizeof(what), "take() with another %s gives null", e.first);
            std::unique_ptr<Payload> got = g_gz->take(e.second);
            check(!got, what);
            if (got) (void)g_gz->give(key, std::move(got));
        }
        std::unique_ptr<Payload> got = g_gz->take(GzKey(0, aqcgz::OffloadOpts{4u << 20, true, 6, 1, 512, true}));
        check(got.get() == p, "take() with an equal key returns that very object");
        check(!g_gz->take(key), "... once");
        check(!g_gz->give(key, std::move(got)), "and it is kept again (to stay until the process ends)");
        // what offload_opts() makes of the environment is part of the key
        unsetenv("AQC_GZ_RESIDENT"); unsetenv("AQC_GZ_RATIO"); unsetenv("AQC_GZ_TOK_RATIO");
        const aqcgz::OffloadOpts d = aqcgz::offload_opts(96u << 20);
        check(d == aqcgz::OffloadOpts{} && d.group_bytes == (96u << 20), "offload_opts(): the defaults");
        check(aqcgz::offload_opts(1).group_bytes == (1u << 20) && aqcgz::offload_opts((size_t)1 << 40).group_bytes == (448u << 20), "offload_opts(): groups of 1 MiB ... 448 MiB");
        setenv("AQC_GZ_RESIDENT", "0", 1);
        check(!(aqcgz::offload_opts(96u << 20) == d) && !aqcgz::offload_opts(96u << 20).resident, "AQC_GZ_RESIDENT=0 is another key");
        unsetenv("AQC_GZ_RESIDENT"); setenv("AQC_GZ_RATIO", "1000", 1);
        check(aqcgz::offload_opts(96u << 20).ratio_cap == 64, "AQC_GZ_RATIO is clamped to 2 ... 64");
        unsetenv("AQC_GZ_RATIO"); setenv("AQC_GZ_TOK_RATIO", "0", 1);
        check(aqcgz::offload_opts(96u << 20).tok_ratio == 1, "AQC_GZ_TOK_RATIO is clamped to 1 ... 16");
        unsetenv("AQC_GZ_TOK_RATIO");
    }
    // ---- the cap --------------------------------------------------------------------------------------------------------------------
    {
        bool all_kept = true;
        for (int i = 0; i < 16; ++i) all_kept = !g_cap->give(i % 3, std::unique_ptr<Payload>(new Payload(100 + i))) && all_kept;
        check(all_kept, "16 objects are kept");
        Payload* p17 = new Payload(116);
        std::unique_ptr<Payload> back = g_cap->give(0, std::unique_ptr<Payload>(p17));
        check(back.get() == p17, "the 17th give() returns the object to the caller");
        const int before = g_destroyed.load();
        back.reset();       // (the caller destroys it, on its own thread)
        g_destroyed_by_test += 1;
        check(g_destroyed.load() == before + 1, "... who destroys it");
        int n = 0;
        std::vector<std::unique_ptr<Payload>> out;
        for (int k = 0; k < 3; ++k)
            while (std::unique_ptr<Payload> q = g_cap->take(k)) { ++n; out.push_back(std::move(q)); }
        check(n == 16, "and 16 are there to be taken");
        bool again = true;
        for (auto& q : out) { const int k = (q->id - 100) % 3; again = !g_cap->give(k, std::move(q)) && again; }
        check(again, "(kept again)");
    }
    // ---- lend -----------------------------------------------------------------------------------------------------------------------
    {
        int calls = 0;
        auto make = [&] { ++calls; return new Payload(200); };
        Payload* a = g_lend->lend(7, make);
        Payload* b = g_lend->lend(7, make);
        check(a && a == b && calls == 1, "lend() twice with one key calls make() once and returns one pointer");
        check(!g_lend->take(7), "take() never returns a lent object");
        Payload* c = g_lend->lend(8, make);
        check(c && c != a && calls == 2, "another key, another object");
        int failed_calls = 0;
        auto cannot = [&]() -> Payload* { ++failed_calls; return nullptr; };
        check(!g_lend->lend(9, cannot) && !g_lend->lend(9, cannot) && failed_calls == 2, "an object that cannot be made is not remembered: the next one asks again");
        check(!g_lend->give(7, std::unique_ptr<Payload>(new Payload(201))) && g_lend->lend(7, make) == a, "what is given under a lent key does not replace the lent object");
        std::unique_ptr<Payload> given = g_lend->take(7);
        check(given && given->id == 201, "... and is what take() finds");
        (void)g_lend->give(7, std::move(given));
    }
    // ---- eight threads, four keys ---------------------------------------------------------------------------------------------------
    {
        for (int i = 0; i < 8; ++i) (void)g_threads->give(i % 4, std::unique_ptr<Payload>(new Payload(300 + i)));
        const int made_before = g_made.load(), destroyed_before = g_destroyed.load();
        std::atomic<int> wrong_key{0}, shared{0}, refused{0}, got_one{0};
        std::vector<std::thread> th;
        for (int t = 0; t < 8; ++t)
            th.emplace_back([&, t] {
                for (int i = 0; i < 1000; ++i) {
                    const int key = (t + i) % 4;
                    std::unique_ptr<Payload> p = g_threads->take(key);
                    if (!p) continue;
                    got_one++;
                    if ((p->id - 300) % 4 != key) wrong_key++;
                    if (p->users.fetch_add(1) != 0) shared++;
                    std::this_thread::yield();
                    p->users.fetch_sub(1);
                    if (g_threads->give(key, std::move(p))) refused++;
                }
            });
        for (auto& x : th) x.join();
        int seen[8] = {};
        int n = 0;
        std::vector<std::unique_ptr<Payload>> out;
        for (int k = 0; k < 4; ++k)
            while (std::unique_ptr<Payload> q = g_threads->take(k)) {
                if (q->id >= 300 && q->id < 308 && (q->id - 300) % 4 == k) seen[q->id - 300]++;
                ++n;
                out.push_back(std::move(q));
            }
        bool each_once = true;
        for (int s : seen) each_once = each_once && s == 1;
        printf("threads: %d takes found an object\n", got_one.load());
        check(n == 8 && each_once, "8 threads x 1000 take() / give() on 4 keys: the 8 objects are all there, each once, under its key");
        check(wrong_key.load() == 0 && shared.load() == 0 && refused.load() == 0 && got_one.load() > 0, "no object under a wrong key, none in two hands, none refused");
        check(g_made.load() == made_before && g_destroyed.load() == destroyed_before, "none made, none destroyed");
        for (auto& q : out) { const int k = (q->id - 300) % 4; (void)g_threads->give(k, std::move(q)); }
    }
    check(g_destroyed.load() == g_destroyed_by_test && g_made.load() - g_destroyed.load() == 1 + 16 + 3 + 8, "28 objects are kept or lent when main() returns, none of them destroyed");
    if (failures) { printf("%d keeper checks FAILED\n", failures); return 1; }
    printf("all keeper checks passed\n");
    return 0;
}
