// aqc_gunzip_offload.hip — gzip INPUT on the device: the threaded host driver of the kernels in aqc_gunzip_dev.hpp.
//
// DeviceInflate is the SectionOffload of aqc_gz.hpp that the pipe's ParallelGunzip hands groups of sections to
// (aqcgz::make_device_offload); aqc_gunzip_dev is the C entry that decodes one whole file with it, aqc_gunzip_probe the one that
// runs ONE group and ONE resolve of it (or of its CPU emulation, aqc_gunzip_ref.hpp) for the tests.  A unit of its own: of the
// C ABI it needs only the page-locked host memory (aqc_host_alloc) and the NUMA helpers, and aqc_gunzip_dev.hpp is the one
// kernel header that includes no other, so its kernels are defined in this unit alone.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "aqc_dev.hpp"
#include "aqc_gunzip_dev.hpp"
#include "aqc_gunzip_ref.hpp"
#include "aqc_gz.hpp"
#include "aqc_keep.hpp"
#include <zlib.h>

using namespace aqc;

// DeviceInflate: the SectionOffload of aqc_gz.hpp.  A group of consecutive sections = one window of the compressed file = one
// pass of scan -> compact -> decode -> chain -> gather.
//
// Round 6.  (1) What a group needs on the device is sized by NEED, not by the worst case: symbols for 6 x its compressed bytes
// (FASTQ expands 3 - 5 x; rounds 4 - 5: 12 x), token entries for 1 per compressed byte + 512 per lane (FASTQ: 0.5 - 0.6 per byte;
// they used to share the symbols' 12 x), one set of decode buffers per decoder instead of one per lane — 2.3 GB for groups of 62 MiB where there were
// two lanes of 9.5 - 10 GB — and they are allocated in the BACKGROUND when the stream announces its group size (prepare()):
// ready() stays false until they exist, so the pool keeps every section until then and nobody waits for a hipMalloc (16 ms per
// GB).  A group that overflows the lean budget comes back short, the host decodes what is missing, and the budgets double for the
// groups after it.  (2) The two lane threads share the decode buffers: one copies its group's compressed bytes out of the file
// mapping into its page-locked stage while the other's kernels run.  (3) RESIDENT results (the default): the sections' symbols
// stay in HBM, in a result set the sections hold until they are dropped; when the consumer arrives with the window before a run
// of them, resolve() turns the symbols into text and computes the CRC-32 of every section there (gzb_windows_kernel,
// gzb_resolve_kernel, gzb_crc_kernel) and fetch() copies text straight to where the consumer wants it.  PCIe carries one byte per
// byte of text instead of two, and the host's 2.2 CPU-seconds per 10 M reads of marker translation + CRC-32 are gone.
// AQC_GZ_RESIDENT=0: the symbols come back into page-locked arenas and the host translates them, as in rounds 4 - 5.

// (C names, exported: an unnamed namespace opened inside an extern "C" block gave the two counters these names in the library's
//  dynamic symbol table when they were added, and that table is kept as it is)
extern "C" {
std::atomic<uint64_t> g_gzb_stats[8];
std::atomic<uint64_t> g_gzb_resolve_stats[4];       // runs resolved, their sections, microseconds in resolve(), bytes of text resolved
}

namespace {

constexpr size_t GZB_SLACK = 4u << 20;              // compressed bytes uploaded behind the last section's stop bit (its last block ends there)

class DeviceInflate : public aqcgz::SectionOffload {
public:
    // Everything it is built with comes in `o` (aqcgz::offload_opts: the defaults and the environment; aqc_gunzip_probe: the
    // budgets a test names, with grow off — a group that comes back short is then not decoded again with more room, and what the
    // test sees is one pass of the kernels).  Nothing here reads the environment for them: (device, o) is the key it is kept under.
    DeviceInflate(int device, const aqcgz::OffloadOpts& o)
        : device_(device), group_bytes_(o.group_bytes), resident_(o.resident), ratio_(o.ratio_cap), tok_ratio_(o.tok_ratio), overlap_tokens_(o.overlap_tokens), grow_(o.grow) {}
    // (runs when a pipe drops a decoder that gave up or that the keeper had no room for — never at exit(): aqc_keep.hpp)
    ~DeviceInflate() override {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& l : lanes_) if (l.th.joinable()) l.th.join();
        (void)hipSetDevice(device_);
        const double t0 = now_s();
        if (dev_.stream) (void)hipStreamSynchronize(dev_.stream);
        if (rs_stream_) (void)hipStreamSynchronize(rs_stream_);
        dev_.release();
        for (auto& r : res_) { r.sym.release(); r.text.release(); }
        rs_wins_.release(); rs_tab_.release(); rs_crc_tab_.release();
        if (rs_stream_) (void)hipStreamDestroy(rs_stream_);
        for (auto& l : lanes_) if (l.stage) aqc_host_free(l.stage);
        if (rs_pin_) aqc_host_free(rs_pin_);
        const double t1 = now_s();
        for (auto& a : arenas_) if (a.p) aqc_host_free(a.p);
        if (debug()) fprintf(stderr, "[gz dev %d] tear-down: device buffers + stages %.3f s, arenas %.3f s\n", device_, t1 - t0, now_s() - t1);
    }
    bool start() {
        if (hipSetDevice(device_) != hipSuccess) { (void)hipGetLastError(); return false; }
        // (the lowest stream priority: where a decoder slice and a kernel of the filter compete for the chip, the filter goes first;
        //  the resolve stream, which the consumer WAITS for, gets the highest)
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        int prio_dec = prio_lo;
        if (const char* e = getenv("AQC_GZ_PRIO")) { if (e[0] == '0') prio_dec = 0; else if (e[0] == '2') prio_dec = prio_hi; }      // (experiments: 0 normal, 2 highest)
        if (hipStreamCreateWithPriority(&dev_.stream, hipStreamNonBlocking, prio_dec) != hipSuccess) return false;
        for (auto& e : dev_.ev) if (hipEventCreate(&e) != hipSuccess) return false;
        if (hipStreamCreateWithPriority(&rs_stream_, hipStreamNonBlocking, prio_hi) != hipSuccess) return false;
        for (int i = 0; i < N_LANES; ++i) lanes_[i].th = std::thread([this, i] { loop(i); });
        return true;
    }
    size_t group_bytes() const override { return group_bytes_; }
    bool ready() override {
        std::lock_guard<std::mutex> g(mu_);
        if (broken_ || stop_ || !prepared_) return false;
        for (auto& l : lanes_) if (!l.job) return true;
        return false;
    }
    bool gave_up() override {
        std::lock_guard<std::mutex> g(mu_);
        return broken_ || stop_;
    }
    // the stream's groups will be about this big: the decode buffers are set up by a lane thread, ready() is false until they are
    void prepare(size_t group_bytes) override {
        {
            std::lock_guard<std::mutex> g(mu_);
            const size_t want = std::min(group_bytes, group_bytes_);
            if (prepared_ && want <= prepared_for_) return;
            if (want > prepare_want_) prepare_want_ = want;
            // (a decoder that has worked before takes groups at once and grows its buffers on the way, as it always did)
            if (prepared_for_ == 0 && !prepare_busy_) prepared_ = false;
        }
        cv_.notify_all();
    }
    bool submit(const uint8_t* data, size_t size, int n, const uint64_t* nominal, const uint64_t* stop, const uint8_t* exact,
                std::function<void(int, const aqcgz::OffloadResult&)> done) override {
        if (n <= 0) return false;
        std::unique_ptr<Group> gr(new Group());
        gr->data = data; gr->size = size; gr->n = n;
        gr->nominal.assign(nominal, nominal + n); gr->stop.assign(stop, stop + n); gr->exact.assign(exact, exact + n);
        gr->done = std::move(done);
        // one window: from the first section's nominal start to the last one's stop bit (+ slack); bit positions are 32-bit inside it
        const uint64_t byte0 = (nominal[0] >> 3) & ~(uint64_t)15;
        const uint64_t last = (stop[n - 1] >> 3) + 1;
        if (stop[n - 1] == UINT64_MAX || last <= byte0 || last - byte0 + GZB_SLACK >= (500u << 20)) return false;
        {
            std::lock_guard<std::mutex> g(mu_);
            if (broken_ || stop_) return false;
            Lane* pick = nullptr;
            for (auto& l : lanes_) if (!l.job) { pick = &l; break; }
            if (!pick) return false;
            pick->job = std::move(gr);
        }
        cv_.notify_all();
        return true;
    }
    void release(void* token) override {
        Token* t = (Token*)token;
        {
            std::lock_guard<std::mutex> g(mu_);
            if (t->res >= 0) res_[t->res].refs--;
            else arenas_[t->arena].refs--;
        }
        cv_.notify_all();
        delete t;
    }

    // ---- resident results: the consumer has arrived with the window before a run of this decoder's sections ----------------------
    const uint8_t* text_ptr(void* token, int* device) override {
        const Token* t = (const Token*)token;
        if (t->res < 0) return nullptr;
        Res& R = res_[t->res];
        if (t->k < 0 || (size_t)t->k >= R.nsym.size()) return nullptr;
        if (device) *device = device_;
        return (const uint8_t*)R.text.p + R.off[(size_t)t->k];
    }
    int resolve(void* const* tokens, int n, const uint8_t* win, size_t wlen, uint32_t* crc, uint8_t* tail, size_t* tail_len, uint32_t* piece_nl) override {
        if (n <= 0 || wlen > GZB_WINDOW) return -2;
        const double t0 = now_s();
        std::lock_guard<std::mutex> rg(rs_mu_);
        if (hipSetDevice(device_) != hipSuccess) { (void)hipGetLastError(); return -2; }
        const Token* t0k = (const Token*)tokens[0];
        if (t0k->res < 0) return -2;
        Res& R = res_[t0k->res];
        // the run's table: first symbol and length of each section, then the CRC pieces (64 KiB, right-aligned in their section)
        uint32_t n_pieces = 0, max_n = 0;
        uint64_t total = 0;
        for (int k = 0; k < n; ++k) {
            const Token* t = (const Token*)tokens[k];
            if (t->res != t0k->res || t->k < 0 || (size_t)t->k >= R.nsym.size()) return -2;
            const uint32_t ns = R.nsym[(size_t)t->k];
            n_pieces += (ns + GZB_CRC_PIECE - 1u) / GZB_CRC_PIECE;
            max_n = std::max(max_n, ns);
            total += ns;
        }
        // device side of the table: off[n] (u64) | nsym[n] | piece_sec[P] | piece_idx[P] | piece_crc[P] | piece_nl[P] | bad
        const size_t o_nsym = 8ull * n, o_psec = o_nsym + 4ull * n, o_pidx = o_psec + 4ull * n_pieces, o_pcrc = o_pidx + 4ull * n_pieces, o_pnl = o_pcrc + 4ull * n_pieces,
                     o_bad = o_pnl + 4ull * n_pieces;
        const size_t tab_bytes = (o_bad + 4 + 15) & ~(size_t)15;
        const size_t pin_need = tab_bytes + GZB_WINDOW * 2;
        if (rs_pin_cap_ < pin_need) {
            if (rs_pin_) aqc_host_free(rs_pin_);
            rs_pin_cap_ = pin_need + pin_need / 2 + (1u << 20);
            rs_pin_ = (uint8_t*)aqc_host_alloc(rs_pin_cap_);
            if (!rs_pin_) { rs_pin_cap_ = 0; return -2; }
        }
        if (rs_tab_.reserve(tab_bytes) || rs_wins_.reserve((size_t)(n + 1) * GZB_WINDOW)) { (void)hipGetLastError(); return -2; }
        if (!rs_crc_tab_.p) {
            uint32_t tab[GZB_CRC_TAB_WORDS];
            auto advance = [](uint32_t x, uint64_t len) { return (uint32_t)crc32_combine((uLong)x, 0UL, (z_off_t)len); };
            gzb_crc_tables(tab, advance);
            for (int j = 0; j < 32; ++j) adv_piece_[j] = advance(1u << j, GZB_CRC_PIECE);
            if (rs_crc_tab_.reserve(sizeof(tab)) || hipMemcpy(rs_crc_tab_.p, tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); rs_crc_tab_.release(); return -2; }
        }
        uint8_t* const pin = rs_pin_;
        uint64_t* const h_off = (uint64_t*)pin;
        uint32_t* const h_nsym = (uint32_t*)(pin + o_nsym);
        uint32_t* const h_psec = (uint32_t*)(pin + o_psec);
        uint32_t* const h_pidx = (uint32_t*)(pin + o_pidx);
        {
            uint32_t p = 0;
            for (int k = 0; k < n; ++k) {
                const Token* t = (const Token*)tokens[k];
                h_off[k] = R.off[(size_t)t->k];
                h_nsym[k] = R.nsym[(size_t)t->k];
                const uint32_t cnt = (h_nsym[k] + GZB_CRC_PIECE - 1u) / GZB_CRC_PIECE;
                for (uint32_t i = 0; i < cnt; ++i, ++p) { h_psec[p] = (uint32_t)k; h_pidx[p] = i; }
            }
            *(uint32_t*)(pin + o_bad) = 0;
        }
        uint8_t* const h_win = pin + tab_bytes;                 // the window before the run, right-aligned; behind it the one behind the run comes back
        memset(h_win, 0, GZB_WINDOW - wlen);
        if (wlen) memcpy(h_win + GZB_WINDOW - wlen, win, wlen);
        GzbResolveJob J{};
        uint8_t* const dtab = (uint8_t*)rs_tab_.p;
        J.sym = (const uint16_t*)R.sym.p; J.text = (uint8_t*)R.text.p; J.wins = (uint8_t*)rs_wins_.p;
        J.off = (const uint64_t*)dtab; J.nsym = (const uint32_t*)(dtab + o_nsym); J.n_run = (uint32_t)n;
        J.valid0 = (uint32_t)(GZB_WINDOW - wlen); J.bad = (uint32_t*)(dtab + o_bad);
        J.piece_sec = (const uint32_t*)(dtab + o_psec); J.piece_idx = (const uint32_t*)(dtab + o_pidx); J.piece_crc = (uint32_t*)(dtab + o_pcrc);
        J.piece_nl = (uint32_t*)(dtab + o_pnl);
        J.n_pieces = n_pieces; J.crc_tab = (const uint32_t*)rs_crc_tab_.p;
        bool ok = hipMemcpyAsync(dtab, pin, tab_bytes, hipMemcpyHostToDevice, rs_stream_) == hipSuccess &&
                  hipMemcpyAsync(rs_wins_.p, h_win, GZB_WINDOW, hipMemcpyHostToDevice, rs_stream_) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(gzb_windows_kernel, dim3(1), dim3(GZB_WIN_THREADS), 0, rs_stream_, J);
            if (max_n) hipLaunchKernelGGL(gzb_resolve_kernel, dim3((max_n + GZB_RES_THREADS * 16 - 1) / (GZB_RES_THREADS * 16), (unsigned)n), dim3(GZB_RES_THREADS), 0, rs_stream_, J);
            if (n_pieces) hipLaunchKernelGGL(gzb_crc_kernel, dim3(n_pieces), dim3(GZB_CRC_THREADS), 0, rs_stream_, J);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyAsync(pin + o_pcrc, dtab + o_pcrc, 8ull * n_pieces + 4, hipMemcpyDeviceToHost, rs_stream_) == hipSuccess &&
                 hipMemcpyAsync(h_win + GZB_WINDOW, (uint8_t*)rs_wins_.p + (size_t)n * GZB_WINDOW, GZB_WINDOW, hipMemcpyDeviceToHost, rs_stream_) == hipSuccess &&
                 hipStreamSynchronize(rs_stream_) == hipSuccess;
        }
        if (!ok) {
            (void)hipGetLastError();
            std::lock_guard<std::mutex> g(mu_);
            broken_ = true;
            return -2;
        }
        if (*(const uint32_t*)(pin + o_bad)) return aqcgz::GZ_ERR_DATA;
        {
            auto advance = [](uint32_t x, uint64_t len) { return (uint32_t)crc32_combine((uLong)x, 0UL, (z_off_t)len); };
            const uint32_t* pc = (const uint32_t*)(pin + o_pcrc);
            for (int k = 0; k < n; ++k) {
                const uint32_t cnt = (h_nsym[k] + GZB_CRC_PIECE - 1u) / GZB_CRC_PIECE;
                crc[k] = gzb_crc_fold(pc, cnt, h_nsym[k], adv_piece_, advance);
                pc += cnt;
            }
            if (piece_nl) memcpy(piece_nl, pin + o_pnl, 4ull * n_pieces);
        }
        const size_t tl = (size_t)std::min<uint64_t>(GZB_WINDOW, wlen + total);
        memcpy(tail, h_win + 2 * GZB_WINDOW - tl, tl);
        *tail_len = tl;
        g_gzb_resolve_stats[0] += 1; g_gzb_resolve_stats[1] += (uint64_t)n; g_gzb_resolve_stats[2] += (uint64_t)((now_s() - t0) * 1e6); g_gzb_resolve_stats[3] += total;
        return 0;
    }
    bool fetch(void* token, size_t off, size_t len, uint8_t* dst) override {
        const Token* t = (const Token*)token;
        if (t->res < 0) return false;
        Res& R = res_[t->res];
        if (t->k < 0 || (size_t)t->k >= R.nsym.size() || off + len > R.nsym[(size_t)t->k]) return false;
        if (!len) return true;
        if (hipSetDevice(device_) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (hipMemcpyAsync(dst, (const uint8_t*)R.text.p + R.off[(size_t)t->k] + off, len, hipMemcpyDeviceToHost, rs_stream_) != hipSuccess) { (void)hipGetLastError(); return false; }
        return true;
    }
    bool fetch_wait() override {
        if (hipSetDevice(device_) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (hipStreamSynchronize(rs_stream_) != hipSuccess) { (void)hipGetLastError(); return false; }
        return true;
    }

private:
    // (two lane threads share ONE set of decode buffers: a group's compressed bytes are copied out of the file mapping into the
    //  lane's stage while the other lane's kernels run; the device part of a group takes the set for itself)
    static constexpr int N_LANES = 2, N_ARENAS = 6, N_RES = 12;
    // AQC_GZ_DEBUG=1: what the decoder's set-up and tear-down cost (device buffers, page-locked staging and arenas), on stderr
    static bool debug() { static const bool d = getenv("AQC_GZ_DEBUG") && getenv("AQC_GZ_DEBUG")[0] == '1'; return d; }
    static double now_s() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
    struct Group {
        const uint8_t* data; size_t size; int n;
        std::vector<uint64_t> nominal, stop;
        std::vector<uint8_t> exact;
        std::function<void(int, const aqcgz::OffloadResult&)> done;
    };
    struct Token { int arena; int res; int k; };
    struct Arena { uint8_t* p = nullptr; size_t cap = 0; int refs = 0; bool filling = false; };
    // a group's symbols and, once resolved, its text (text[i] = the byte of symbol i): kept until the last of its sections is dropped
    struct Res {
        DevBuf sym, text;
        std::vector<uint64_t> off;
        std::vector<uint32_t> nsym;
        int refs = 0;
        bool filling = false;
    };
    struct Lane {
        std::thread th;
        std::unique_ptr<Group> job;
        uint8_t* stage = nullptr;          // page-locked copy of the group's compressed bytes (the file itself is a pageable mapping)
        size_t stage_cap = 0;
    };
    struct DevSet {
        hipStream_t stream = nullptr;
        hipEvent_t ev[7] = {};
        DevBuf comp, tile_cnt, tile_cand, n_cand, c_start, c_end, c_nsym, c_flags, c_symoff, c_symcap, c_tokoff, c_tokcap, blk_sym, tables, blk_tp, c_lanes, l_u32;
        DevBuf s_in, s_out, s_blocks, s_sym, s_off;
        std::vector<DevBuf*> all() {
            return {&comp, &tile_cnt, &tile_cand, &n_cand, &c_start, &c_end, &c_nsym, &c_flags, &c_symoff, &c_symcap, &c_tokoff, &c_tokcap, &blk_sym, &tables, &blk_tp, &c_lanes, &l_u32,
                    &s_in, &s_out, &s_blocks, &s_sym, &s_off};
        }
        size_t bytes() { size_t t = 0; for (DevBuf* x : all()) t += x->cap; return t; }
        void release() {
            for (DevBuf* x : all()) x->release();
            for (auto& e : ev) if (e) (void)hipEventDestroy(e);
            if (stream) (void)hipStreamDestroy(stream);
            stream = nullptr;
        }
    };
    struct Sizes { uint32_t n_tiles, cand_cap, s_symcap; uint64_t blk_sym_cap, blk_tp_cap, s_sym_total; };
    Sizes sizes_for(size_t span, int n, uint64_t sec_max, uint32_t last_bit) const {
        Sizes z;
        z.n_tiles = (uint32_t)(((size_t)(last_bit >> 3) + 1 + GZB_SCAN_TILE - 1) / GZB_SCAN_TILE);
        z.cand_cap = (uint32_t)(span / 4096 + 256);
        z.s_symcap = (uint32_t)std::min<uint64_t>((sec_max * 2 * ratio_ + (2u << 20) + 7) & ~(uint64_t)7, 0xfffffff0u);
        z.blk_sym_cap = gzb_sym_budget(span, ratio_);
        z.blk_tp_cap = gzb_tok_budget(span, tok_ratio_, overlap_tokens_);
        z.s_sym_total = (uint64_t)span * ratio_ + (uint64_t)n * 64 + (1u << 20);
        return z;
    }
    // the decode buffers for a window of `span` compressed bytes in n sections (grow only; dev_mu_ held)
    bool reserve_devset(size_t span, int n, const Sizes& z) {
        DevSet& D = dev_;
        const double t0 = now_s();
        const size_t before = D.bytes();
        if (D.comp.reserve(span + 512) || D.tile_cnt.reserve(4ull * z.n_tiles) || D.tile_cand.reserve(4ull * z.n_tiles * GZB_TILE_CAND) || D.n_cand.reserve(64) ||
            D.c_start.reserve(4ull * z.cand_cap) || D.c_end.reserve(4ull * z.cand_cap) || D.c_nsym.reserve(4ull * z.cand_cap) || D.c_flags.reserve(4ull * z.cand_cap) ||
            D.c_symoff.reserve(8ull * z.cand_cap) || D.c_symcap.reserve(4ull * z.cand_cap) || D.c_tokoff.reserve(8ull * z.cand_cap) || D.c_tokcap.reserve(4ull * z.cand_cap) ||
            D.blk_sym.reserve(2ull * z.blk_sym_cap + 64) || D.blk_tp.reserve(8ull * z.blk_tp_cap + 512) || D.c_lanes.reserve(4ull * z.cand_cap) ||
            D.l_u32.reserve(5ull * 4ull * z.cand_cap * GZB_K) || D.tables.reserve(4ull * z.cand_cap * GZB_TAB_WORDS) || D.s_in.reserve(12ull * n) || D.s_out.reserve(16ull * n) ||
            D.s_off.reserve(8ull * (n + 1)) || D.s_blocks.reserve(12ull * n * GZB_SEC_BLOCKS) || (!resident_ && D.s_sym.reserve(2ull * z.s_sym_total + 64)))
            return false;
        if (debug() && D.bytes() != before)
            fprintf(stderr, "[gz dev %d] decode buffers for %.1f MiB compressed in %d sections (symbols %u x, tokens %u per byte): %.2f GiB (blk_sym %.2f, blk_tp %.2f, tables %.2f, s_sym %.2f), reserve %.3f s\n",
                    device_, span / 1048576.0, n, ratio_, tok_ratio_, D.bytes() / 1073741824.0, D.blk_sym.cap / 1073741824.0, D.blk_tp.cap / 1073741824.0, D.tables.cap / 1073741824.0,
                    D.s_sym.cap / 1073741824.0, now_s() - t0);
        return true;
    }
    bool reserve_stage(Lane& L, size_t span) {
        if (L.stage_cap >= span) return true;
        if (L.stage) aqc_host_free(L.stage);
        L.stage_cap = span + span / 8 + (1u << 20);
        const double t0 = now_s();
        L.stage = (uint8_t*)aqc_host_alloc(L.stage_cap);
        if (debug()) fprintf(stderr, "[gz dev %d] stage: %.0f MiB page-locked in %.3f s\n", device_, L.stage_cap / 1048576.0, now_s() - t0);
        if (!L.stage) { L.stage_cap = 0; return false; }
        return true;
    }

    void loop(int li) {
        Lane& L = lanes_[li];
        (void)hipSetDevice(device_);
        (void)aqc_bind_thread_to_node(aqc_device_numa_node_of(device_));       // (the staging copies and the arenas' first touch happen here)
        for (;;) {
            Group* gr = nullptr;
            size_t prep = 0;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || L.job || (!prepare_busy_ && prepare_want_ > prepared_for_); });
                if (stop_ && !L.job) return;
                if (L.job) gr = L.job.get();
                else { prep = prepare_want_; prepare_busy_ = true; }
            }
            if (!gr) {
                // the stream has announced its groups: the decode buffers, this lane's stage (the other lane makes its own with its
                // first group) and the first result set, before the first group is accepted
                const size_t span = prep + GZB_SLACK + (1u << 20);
                const int n = (int)(prep / (256u << 10)) + 8;
                bool ok;
                {
                    std::lock_guard<std::mutex> dg(dev_mu_);
                    ok = reserve_devset(span, n, sizes_for(span, n, 2u << 20, (uint32_t)std::min<uint64_t>((uint64_t)span * 8, 0xffffffffu)));
                }
                ok = ok && reserve_stage(L, span);
                if (ok && resident_) {
                    // three result sets of a typical group's size (FASTQ expands 3 - 5 x) — the consumer is seldom further behind;
                    // more are made when they are needed, which then costs the lane that needs one 16 ms per GB
                    int got[3] = {-1, -1, -1};
                    for (int& ri : got) ri = take_res((uint64_t)prep * 4);
                    std::lock_guard<std::mutex> g(mu_);
                    for (int ri : got) if (ri >= 0) res_[ri].filling = false;
                }
                {
                    std::lock_guard<std::mutex> g(mu_);
                    prepare_busy_ = false;
                    prepared_for_ = std::max(prepared_for_, prep);
                    prepared_ = true;
                    if (!ok) { (void)hipGetLastError(); broken_ = true; }
                }
                cv_.notify_all();
                continue;
            }
            if (!run_group(L, *gr)) {
                // the device path failed for this group: the sections come back empty, the host decodes that stretch itself
                (void)hipGetLastError();
                aqcgz::OffloadResult none;
                for (int k = 0; k < gr->n; ++k) gr->done(k, none);
                std::lock_guard<std::mutex> g(mu_);
                broken_ = true;
            }
            {
                std::lock_guard<std::mutex> g(mu_);
                L.job.reset();
                prepared_ = true;            // (a decoder that has run a group has its buffers)
                if (prepared_for_ == 0) prepared_for_ = 1;
            }
        }
    }

    // a free arena of at least `need` bytes (waits for one; grows the smallest free one when none is big enough)
    int take_arena(size_t need) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            int best = -1, empty = -1, small = -1;
            for (int i = 0; i < N_ARENAS; ++i) {
                Arena& a = arenas_[i];
                if (a.refs || a.filling) continue;
                if (!a.p) { if (empty < 0) empty = i; continue; }
                if (a.cap >= need) { if (best < 0 || a.cap < arenas_[best].cap) best = i; }
                else if (small < 0) small = i;
            }
            int pick = best >= 0 ? best : (empty >= 0 ? empty : small);
            if (pick >= 0) {
                Arena& a = arenas_[pick];
                a.filling = true;
                if (a.cap < need) {
                    lk.unlock();
                    if (a.p) aqc_host_free(a.p);
                    const size_t want = need + need / 4 + (8u << 20);
                    const double t0 = now_s();
                    a.p = (uint8_t*)aqc_host_alloc(want);
                    if (debug()) fprintf(stderr, "[gz dev %d] arena %d: %.0f MiB page-locked in %.3f s\n", device_, pick, want / 1048576.0, now_s() - t0);
                    a.cap = a.p ? want : 0;
                    lk.lock();
                    if (!a.p) { a.filling = false; return -1; }
                }
                return pick;
            }
            if (stop_) return -1;
            cv_.wait(lk);
        }
    }
    // a free result set for `need` symbols (waits for one; the best fit, else an empty one, else the smallest grows).  The consumer
    // holds at most four groups' worth of sections of a stream (ParallelGunzip::top_up), the chunks on their way to the slots a few
    // more (the pipe's ring: five chunks of ~45 MB), and there are two lanes: twelve never run out.
    int take_res(uint64_t need) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            int best = -1, empty = -1, small = -1;
            for (int i = 0; i < N_RES; ++i) {
                Res& r = res_[i];
                if (r.refs || r.filling) continue;
                if (!r.sym.p) { if (empty < 0) empty = i; continue; }
                if (r.sym.cap >= 2 * need + 64 && r.text.cap >= need + 64) { if (best < 0 || r.sym.cap < res_[best].sym.cap) best = i; }
                else if (small < 0 || r.sym.cap > res_[small].sym.cap) small = i;
            }
            const int pick = best >= 0 ? best : (empty >= 0 ? empty : small);
            if (pick >= 0) {
                Res& r = res_[pick];
                r.filling = true;
                if (r.sym.cap < 2 * need + 64 || r.text.cap < need + 64) {
                    lk.unlock();
                    const double t0 = now_s();
                    const bool bad = r.sym.reserve(2 * need + 64) || r.text.reserve(need + 64);
                    if (debug()) fprintf(stderr, "[gz dev %d] result set %d: %.2f GiB (symbols + text of %.0f M symbols) in %.3f s\n", device_, pick, (r.sym.cap + r.text.cap) / 1073741824.0, need / 1e6, now_s() - t0);
                    lk.lock();
                    if (bad) { (void)hipGetLastError(); r.filling = false; return -1; }
                }
                return pick;
            }
            if (stop_) return -1;
            cv_.wait(lk);
        }
    }

#define GZB_TRY(expr) do { if ((expr) != hipSuccess) return false; } while (0)
    bool run_group(Lane& L, Group& G) {
        const int n = G.n;
        const uint64_t byte0 = (G.nominal[0] >> 3) & ~(uint64_t)15;
        const uint64_t end_byte = std::min<uint64_t>(G.size, (G.stop[n - 1] >> 3) + 1 + GZB_SLACK);
        const size_t span = (size_t)(end_byte - byte0);
        const uint32_t first_bit = (uint32_t)(G.nominal[0] - byte0 * 8), last_bit = (uint32_t)std::min<uint64_t>(G.stop[n - 1] - byte0 * 8, (uint64_t)span * 8);
        uint64_t sec_max = 0;
        for (int k = 0; k < n; ++k) sec_max = std::max<uint64_t>(sec_max, (G.stop[k] - G.nominal[k]) >> 3);
        // the compressed bytes: out of the (pageable, possibly not yet faulted-in) file mapping into page-locked memory with a few
        // threads side by side, then one DMA — a copy straight from the mapping runs at the page-fault rate of one thread.  (Before
        // the decode buffers are taken: the other lane's kernels run meanwhile.)
        if (!reserve_stage(L, span)) return false;
        {
            const int T = span > (8u << 20) ? 4 : 1;
            std::vector<std::thread> th;
            const size_t per = (span + T - 1) / T;
            for (int t = 1; t < T; ++t)
                th.emplace_back([&, t] { const size_t a = std::min(span, t * per), b = std::min(span, a + per); memcpy(L.stage + a, G.data + byte0 + a, b - a); });
            memcpy(L.stage, G.data + byte0, std::min(span, per));
            for (auto& x : th) x.join();
        }
        // section table: nominal, stop, exact (bits relative to the window)
        std::vector<uint32_t> sin(3 * (size_t)n);
        for (int k = 0; k < n; ++k) {
            sin[k] = (uint32_t)(G.nominal[k] - byte0 * 8);
            sin[n + k] = (uint32_t)std::min<uint64_t>(G.stop[k] - byte0 * 8, (uint64_t)span * 8);
            sin[2 * n + k] = G.exact[k];
        }
        std::unique_lock<std::mutex> dg(dev_mu_);
        DevSet& D = dev_;
      for (int attempt = 0;; ++attempt) {
        const Sizes z = sizes_for(span, n, sec_max, last_bit);
        if (!reserve_devset(span, n, z)) return false;
        GZB_TRY(hipEventRecord(D.ev[0], D.stream));
        GZB_TRY(hipMemcpyAsync(D.comp.p, L.stage, span, hipMemcpyHostToDevice, D.stream));
        GZB_TRY(hipMemsetAsync((uint8_t*)D.comp.p + span, 0, 512, D.stream));       // (the lanes' stream windows read up to 200 bytes ahead)
        GZB_TRY(hipMemcpyAsync(D.s_in.p, sin.data(), 12ull * n, hipMemcpyHostToDevice, D.stream));
        GzbJob J{};
        J.comp = (const uint8_t*)D.comp.p; J.comp_bytes = (uint32_t)span; J.scan_byte0 = 0; J.first_bit = first_bit; J.last_bit = last_bit;
        J.n_tiles = z.n_tiles; J.tile_cnt = (uint32_t*)D.tile_cnt.p; J.tile_cand = (uint32_t*)D.tile_cand.p;
        J.cand_cap = z.cand_cap; J.n_cand = (uint32_t*)D.n_cand.p;
        J.c_start = (uint32_t*)D.c_start.p; J.c_end = (uint32_t*)D.c_end.p; J.c_nsym = (uint32_t*)D.c_nsym.p; J.c_flags = (uint32_t*)D.c_flags.p;
        J.c_symoff = (uint64_t*)D.c_symoff.p; J.c_symcap = (uint32_t*)D.c_symcap.p; J.blk_sym = (uint16_t*)D.blk_sym.p; J.blk_sym_cap = z.blk_sym_cap;
        J.c_tokoff = (uint64_t*)D.c_tokoff.p; J.c_tokcap = (uint32_t*)D.c_tokcap.p; J.blk_tp_cap = z.blk_tp_cap; J.tok_ratio = tok_ratio_; J.overlap_tokens = overlap_tokens_;
        J.ratio_cap = ratio_; J.tables = (uint32_t*)D.tables.p; J.blk_tp = (unsigned long long*)D.blk_tp.p;
        J.c_lanes = (uint32_t*)D.c_lanes.p;
        J.l_p = (uint32_t*)D.l_u32.p; J.l_stop = J.l_p + (size_t)z.cand_cap * GZB_K; J.l_start = J.l_stop + (size_t)z.cand_cap * GZB_K;
        J.l_ntok = J.l_start + (size_t)z.cand_cap * GZB_K; J.l_flags = J.l_ntok + (size_t)z.cand_cap * GZB_K;
        {
            static const uint32_t slice = [] { const char* e = getenv("AQC_GZ_SLICE"); return e ? (uint32_t)std::max(16, atoi(e)) : 2048u; }();
            J.slice_tokens = slice;
        }
        J.n_sec = (uint32_t)n; J.s_nominal = (const uint32_t*)D.s_in.p; J.s_stop = J.s_nominal + n; J.s_exact = J.s_nominal + 2 * n;
        J.s_start = (uint32_t*)D.s_out.p; J.s_end = J.s_start + n; J.s_nsym = J.s_start + 2 * n; J.s_nblk = J.s_start + 3 * n;
        J.s_blocks = (uint32_t*)D.s_blocks.p; J.s_off = (uint64_t*)D.s_off.p; J.s_sym = (uint16_t*)D.s_sym.p; J.s_symcap = z.s_symcap;
        // (resident: the result set is taken once the sections' sizes are known, so every section that chained up has its place)
        J.s_sym_total = resident_ ? ~0ull >> 2 : z.s_sym_total;
        GZB_TRY(hipEventRecord(D.ev[1], D.stream));
        hipLaunchKernelGGL(gzb_scan_kernel, dim3(z.n_tiles), dim3(GZB_SCAN_THREADS), 0, D.stream, J);
        hipLaunchKernelGGL(gzb_compact_kernel, dim3(1), dim3(1024), 0, D.stream, J);
        GZB_TRY(hipEventRecord(D.ev[2], D.stream));
        // the decoder in slices (aqc_gunzip_dev.hpp): GZB_K lanes per block, each with its share of it and the overlap: 6 x 2048
        // tokens cover the blocks of zlib (<= 16 K tokens) and of GNU gzip (<= 32 K) with room to spare; a lane that needs more
        // stays unfinished, its block counts as failed, the section ends before it and the host goes on from there
        {
            static const int n_slices = [] { const char* e = getenv("AQC_GZ_SLICES"); return e ? std::max(1, atoi(e)) : 6; }();
            hipLaunchKernelGGL(gzb_tables_kernel, dim3((z.cand_cap + GZB_DEC_THREADS - 1) / GZB_DEC_THREADS), dim3(GZB_DEC_THREADS), 0, D.stream, J);
            const dim3 grid((z.cand_cap * GZB_K + GZB_DEC_THREADS - 1) / GZB_DEC_THREADS);
            for (int sl = 0; sl < n_slices; ++sl) hipLaunchKernelGGL(gzb_decode_kernel, grid, dim3(GZB_DEC_THREADS), 0, D.stream, J);
            // phase 2: a wave per block stitches its lanes' lists together and applies the tokens
            hipLaunchKernelGGL(gzb_expand_kernel, dim3((z.cand_cap + GZB_EXP_WAVES - 1) / GZB_EXP_WAVES), dim3(64 * GZB_EXP_WAVES), 0, D.stream, J);
        }
        GZB_TRY(hipEventRecord(D.ev[3], D.stream));
        hipLaunchKernelGGL(gzb_chain_kernel, dim3((n + 63) / 64), dim3(64), 0, D.stream, J);
        hipLaunchKernelGGL(gzb_place_kernel, dim3(1), dim3(1), 0, D.stream, J);
        GZB_TRY(hipGetLastError());
        // what each section became (start, end, symbols) and where its symbols go
        std::vector<uint32_t> sout(4 * (size_t)n);
        std::vector<uint64_t> soff((size_t)n + 1);
        GZB_TRY(hipMemcpyAsync(sout.data(), D.s_out.p, 16ull * n, hipMemcpyDeviceToHost, D.stream));
        GZB_TRY(hipMemcpyAsync(soff.data(), D.s_off.p, 8ull * (n + 1), hipMemcpyDeviceToHost, D.stream));
        GZB_TRY(hipStreamSynchronize(D.stream));
        int live = 0;
        for (int k = 0; k < n; ++k) if (sout[k] != GZB_NONE && sout[2 * n + k] != 0) ++live;
        // A group that comes back short on the lean budgets (symbols 6 x, one token per compressed byte) is decoded once more with
        // room to spare, and so is every group after it (once per decoder: an input that compresses 6 x and better, or is nearly
        // all literals, is rare — and says so here; what is still missing then is not a matter of space, and the host's)
        if (grow_ && live < n && !grown_) {
            grown_ = true;
            {
                std::lock_guard<std::mutex> g(mu_);
                ratio_ = std::max(ratio_, 12u);
                tok_ratio_ = std::max(tok_ratio_, 6u);
                overlap_tokens_ = std::max(overlap_tokens_, 2048u);
            }
            if (debug()) fprintf(stderr, "[gz dev %d] %d of %d sections came back empty: symbol space %u x, %u tokens per byte from now on; the group is decoded again\n", device_, n - live, n, ratio_, tok_ratio_);
            if (attempt == 0) continue;
        }
        int ai = -1, ri = -1;
        bool ok = true;
        if (resident_) {
            if (soff[n] && live) {
                ri = take_res(soff[n]);
                if (ri < 0) return false;
                J.s_sym = (uint16_t*)res_[ri].sym.p;
                hipLaunchKernelGGL(gzb_gather_kernel, dim3(n), dim3(GZB_GATHER_THREADS), 0, D.stream, J);
            }
            ok = hipEventRecord(D.ev[4], D.stream) == hipSuccess && hipEventRecord(D.ev[6], D.stream) == hipSuccess && hipEventRecord(D.ev[5], D.stream) == hipSuccess &&
                 hipGetLastError() == hipSuccess && hipStreamSynchronize(D.stream) == hipSuccess;
            if (ri >= 0) {
                std::lock_guard<std::mutex> g(mu_);
                Res& R = res_[ri];
                R.filling = false;
                R.refs = ok ? live : 0;
                R.off.assign(soff.begin(), soff.begin() + n);
                R.nsym.assign(sout.begin() + 2 * n, sout.begin() + 3 * n);
            }
        } else {
            hipLaunchKernelGGL(gzb_gather_kernel, dim3(n), dim3(GZB_GATHER_THREADS), 0, D.stream, J);
            ok = hipEventRecord(D.ev[4], D.stream) == hipSuccess;
            const size_t need = (size_t)soff[n] * 2;
            if (ok && need && live) {
                ai = take_arena(need);
                if (ai < 0) return false;
                ok = hipEventRecord(D.ev[6], D.stream) == hipSuccess &&
                     hipMemcpyAsync(arenas_[ai].p, D.s_sym.p, need, hipMemcpyDeviceToHost, D.stream) == hipSuccess;
            } else ok = ok && hipEventRecord(D.ev[6], D.stream) == hipSuccess;
            ok = ok && hipEventRecord(D.ev[5], D.stream) == hipSuccess && hipStreamSynchronize(D.stream) == hipSuccess;
            if (ai >= 0) {
                std::lock_guard<std::mutex> g(mu_);
                arenas_[ai].filling = false;
                arenas_[ai].refs = ok ? live : 0;
            }
        }
        if (!ok) { cv_.notify_all(); return false; }
        float ms[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ms[i], D.ev[i], D.ev[i + 1]);
        (void)hipEventElapsedTime(&ms[4], D.ev[6], D.ev[5]);       // (the symbols' copy alone: getting an arena is host time)
        dg.unlock();
        g_gzb_stats[0] += (uint64_t)(ms[1] * 1000); g_gzb_stats[1] += (uint64_t)(ms[2] * 1000); g_gzb_stats[2] += (uint64_t)(ms[3] * 1000);
        g_gzb_stats[3] += (uint64_t)(ms[0] * 1000); g_gzb_stats[4] += (uint64_t)(ms[4] * 1000); g_gzb_stats[5] += 1; g_gzb_stats[6] += (uint64_t)n; g_gzb_stats[7] += (uint64_t)live;
        for (int k = 0; k < n; ++k) {
            aqcgz::OffloadResult r;
            if (sout[k] != GZB_NONE && sout[2 * n + k] != 0) {
                r.found = true;
                r.start_bit = byte0 * 8 + sout[k];
                r.end_bit = byte0 * 8 + sout[n + k];
                r.n_sym = sout[2 * n + k];
                if (resident_) { r.resident = true; r.token = new Token{-1, ri, k}; }
                else { r.sym = (const uint16_t*)arenas_[ai].p + soff[k]; r.token = new Token{ai, -1, k}; }
            }
            G.done(k, r);
        }
        return true;
      }
    }
#undef GZB_TRY

    int device_;
    size_t group_bytes_;
    bool resident_;
    uint32_t ratio_, tok_ratio_, overlap_tokens_;       // (raised once, when a group comes back short: grow_)
    bool grow_, grown_ = false;
    std::mutex mu_;
    std::condition_variable cv_;
    bool stop_ = false, broken_ = false;
    bool prepared_ = true, prepare_busy_ = false;       // (prepared_: false between prepare() and the moment the buffers it asked for exist)
    size_t prepare_want_ = 0, prepared_for_ = 0;
    Lane lanes_[N_LANES];
    std::mutex dev_mu_;
    DevSet dev_;
    Arena arenas_[N_ARENAS];
    Res res_[N_RES];
    // resolve() / fetch(): the consumer's side
    std::mutex rs_mu_;
    hipStream_t rs_stream_ = nullptr;
    DevBuf rs_wins_, rs_tab_, rs_crc_tab_;
    uint8_t* rs_pin_ = nullptr;
    size_t rs_pin_cap_ = 0;
    uint32_t adv_piece_[32] = {};
};

static_assert(aqcgz::OffloadOpts{}.overlap_tokens == GZB_OVERLAP_TOKENS, "aqc_gz.hpp states the kernels' default");

// The decoders of the two C entries below, lent to their callers for the life of the process (aqc_keep.hpp), a keeper per entry:
// a probe's decoder keeps the budgets it was given, aqc_gunzip_dev's grow — and the pipe's own (aqc_pipe.cpp) have one consumer each.
using GzKey = std::pair<int, aqcgz::OffloadOpts>;
Keep<GzKey, aqcgz::SectionOffload>* const g_dev_keep = new Keep<GzKey, aqcgz::SectionOffload>;
Keep<GzKey, aqcgz::SectionOffload>* const g_probe_keep = new Keep<GzKey, aqcgz::SectionOffload>;

}  // namespace

namespace aqcgz {
SectionOffload* make_device_offload(int device, const OffloadOpts& opts) {
    std::unique_ptr<DeviceInflate> d(new DeviceInflate(device, opts));
    if (!d->start()) { (void)hipGetLastError(); return nullptr; }
    return d.release();
}
void device_offload_stats(uint64_t out[8]) {
    for (int i = 0; i < 8; ++i) out[i] = g_gzb_stats[i].load();
}
void device_resolve_stats(uint64_t out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = g_gzb_resolve_stats[i].load();
}
}  // namespace aqcgz

extern "C" {

// One gzip file decoded with the device taking every section it can (what the pipe does for a `.gz` input, minus the pool's share
// of the sections): `threads` host threads translate symbols and check CRC-32 / ISIZE, the stream's last section and whatever the
// device does not chain up is decoded on the host.  stats: sections committed from the device / from the host, bytes decoded
// sequentially on the host (bridges), then aqcgz::device_offload_stats()[0..5) of this call (microseconds in the scan + compact,
// decode, chain + gather kernels, H2D, D2H).
int aqc_gunzip_dev(int device, const uint8_t* gz, uint64_t size, uint8_t* out, uint64_t cap, uint64_t* n_out, uint64_t stats[8], int threads,
                   uint64_t section_bytes, uint64_t group_bytes) {
    if (!gz || !out || !n_out || !stats) return fail(AQC_ERR_ARG, "null argument");
    // (one decoder per device and set of options for the life of the process: its device buffers and page-locked arenas cost more
    //  to set up than a gigabyte takes to decode)
    const GzKey key(device, aqcgz::offload_opts(group_bytes ? (size_t)group_bytes : (256u << 20)));
    aqcgz::SectionOffload* off = g_dev_keep->lend(key, [&] { return aqcgz::make_device_offload(key.first, key.second); });
    if (!off) return fail(AQC_ERR_HIP, "device gunzip: cannot set up device %d", device);
    uint64_t before[8], after[8];
    aqcgz::device_offload_stats(before);
    aqc_host::Pool pool(threads > 0 ? threads : 0);
    memset(stats, 0, 8 * sizeof(uint64_t));
    uint64_t produced = 0;
    int rc = 0;
    {
        aqcgz::ParallelGunzip pg(gz, (size_t)size, threads > 0 ? &pool : nullptr, std::max(4, 2 * threads), section_bytes ? (size_t)section_bytes : (1u << 20), off, true);
        while (produced < cap) {
            const size_t got = pg.read(out + produced, (size_t)std::min<uint64_t>(cap - produced, 256u << 20));
            if (pg.failed()) { rc = fail(AQC_ERR_ARG, "device gunzip: %s", pg.error()); break; }
            if (!got) break;
            produced += got;
        }
        if (!rc && produced == cap) {
            uint8_t probe;
            if (pg.read(&probe, 1) != 0) rc = fail(AQC_ERR_ARG, "output does not fit");
        }
        stats[0] = pg.offloaded_accepted; stats[1] = pg.sections_accepted - pg.offloaded_accepted; stats[2] = pg.bridged_bytes;
    }
    aqcgz::device_offload_stats(after);
    for (int i = 0; i < 5; ++i) stats[3 + i] = after[i] - before[i];
    *n_out = produced;
    return rc;
}

// One group and one resolve, through SectionOffload's public interface alone: what the tests hold the kernels to (engine 1:
// DeviceInflate with the budgets given and no second attempt) and what they hold them against (engine 0: CpuOffload of
// aqc_gunzip_ref.hpp, the same GZB_HD functions in plain loops, with the same budgets, DeviceInflate's sizing rules and the
// kernels' slice budget).  The sections nominal / stop / exact [n] over gz[0, size) go in as ONE submit(); sec[4 * k ..] = found,
// start_bit, end_bit, n_sym of section k.  The longest run of found sections that chain (end_bit == the next one's start_bit;
// the first of equals) is resolved with win[0, wlen) in front of it: run[0] its first section, run[1] its length (0: nothing was
// found), run[2] resolve()'s status — 0, or the data error of a marker that points before the member's start, after which
// nothing below is filled in.  crc[j], j < run[1]; piece_nl[0, *n_pieces); text[0, *n_text) = the run's sections one after the
// other; tail[0, *tail_len) = the window behind the run (tail: 32768 bytes).
int aqc_gunzip_probe(int engine, int device, const uint8_t* gz, uint64_t size, int n, const uint64_t* nominal, const uint64_t* stop, const uint8_t* exact,
                     uint32_t ratio_cap, uint32_t tok_ratio, uint32_t overlap_tokens, const uint8_t* win, uint64_t wlen, uint64_t* sec, int32_t* run,
                     uint32_t* crc, uint32_t* piece_nl, uint64_t piece_cap, uint64_t* n_pieces, uint8_t* text, uint64_t text_cap, uint64_t* n_text,
                     uint8_t* tail, uint64_t* tail_len) {
    if (!gz || !nominal || !stop || !exact || !sec || !run || !crc || !piece_nl || !n_pieces || !text || !n_text || !tail || !tail_len || (wlen && !win))
        return fail(AQC_ERR_ARG, "null argument");
    if (n <= 0 || wlen > GZB_WINDOW || ratio_cap < 1 || ratio_cap > 4096 || tok_ratio < 1 || tok_ratio > 16 || overlap_tokens < 1 || overlap_tokens > 65536 || (engine != 0 && engine != 1))
        return fail(AQC_ERR_ARG, "gunzip probe: bad argument");
    for (int k = 0; k < n; ++k)
        if (nominal[k] > stop[k] || (stop[k] >> 3) >= size || (k > 0 && nominal[k] < nominal[k - 1])) return fail(AQC_ERR_ARG, "gunzip probe: section %d is not inside the image, or out of order", k);
    static std::mutex mu;       // (one probe at a time: a decoder takes two groups at most, and the done callbacks below are this call's)
    std::lock_guard<std::mutex> lock(mu);
    std::unique_ptr<CpuOffload> cpu;
    aqcgz::SectionOffload* off = nullptr;
    if (engine == 0) {
        cpu.reset(new CpuOffload(1u << 20));
        cpu->resident = true;
        cpu->ratio_cap = ratio_cap; cpu->tok_ratio = tok_ratio; cpu->overlap_tokens = overlap_tokens;
        cpu->slice_tokens = 2048; cpu->max_slices = 6;
        cpu->slack = GZB_SLACK; cpu->sec_ratio = 2 * ratio_cap; cpu->total_unbounded = true;
        off = cpu.get();
    } else {
        // (as aqc_gunzip_dev keeps its decoders: buffers are set up once.  Resident results, the budgets given, no second attempt)
        const GzKey key(device, aqcgz::OffloadOpts{1u << 20, true, ratio_cap, tok_ratio, overlap_tokens, false});
        off = g_probe_keep->lend(key, [&] { return aqcgz::make_device_offload(key.first, key.second); });
        if (!off) return fail(AQC_ERR_HIP, "gunzip probe: cannot set up device %d", device);
    }
    // (1) one group, (2) its done callbacks
    std::vector<aqcgz::OffloadResult> res((size_t)n);
    {
        std::mutex dmu;
        std::condition_variable dcv;
        int pending = n;
        if (!off->submit(gz, (size_t)size, n, nominal, stop, exact, [&](int k, const aqcgz::OffloadResult& r) {
                std::lock_guard<std::mutex> g(dmu);
                res[(size_t)k] = r;
                if (--pending == 0) dcv.notify_all();
            }))
            return fail(AQC_ERR_ARG, "gunzip probe: the decoder does not take the group");
        std::unique_lock<std::mutex> lk(dmu);
        dcv.wait(lk, [&] { return pending == 0; });
    }
    for (int k = 0; k < n; ++k) { sec[4 * k] = res[(size_t)k].found; sec[4 * k + 1] = res[(size_t)k].start_bit; sec[4 * k + 2] = res[(size_t)k].end_bit; sec[4 * k + 3] = res[(size_t)k].n_sym; }
    int best0 = 0, best_n = 0;
    for (int k = 0; k < n;) {
        if (!res[(size_t)k].found) { ++k; continue; }
        int e = k + 1;
        while (e < n && res[(size_t)e].found && res[(size_t)e].start_bit == res[(size_t)e - 1].end_bit) ++e;
        if (e - k > best_n) { best0 = k; best_n = e - k; }
        k = e;
    }
    run[0] = best0; run[1] = best_n; run[2] = 0;
    *n_pieces = 0; *n_text = 0; *tail_len = 0;
    int rc = 0;
    // (3) one resolve over that run, (4) its text
    if (best_n > 0) {
        std::vector<void*> tokens;
        uint64_t total = 0, pieces = 0;
        for (int j = 0; j < best_n; ++j) {
            const aqcgz::OffloadResult& r = res[(size_t)(best0 + j)];
            if (!r.resident || !r.token) { rc = fail(AQC_ERR_ARG, "gunzip probe: the decoder's results are not resident"); break; }
            tokens.push_back(r.token);
            total += r.n_sym;
            pieces += (r.n_sym + GZB_CRC_PIECE - 1u) / GZB_CRC_PIECE;
        }
        if (!rc && (total > text_cap || pieces > piece_cap)) rc = fail(AQC_ERR_ARG, "gunzip probe: %llu bytes of text in %llu pieces do not fit", (unsigned long long)total, (unsigned long long)pieces);
        if (!rc) {
            size_t tl = 0;
            const int st = off->resolve(tokens.data(), best_n, win, (size_t)wlen, crc, tail, &tl, piece_nl);
            run[2] = st;
            if (st == -2) rc = fail(AQC_ERR_HIP, "gunzip probe: resolve() failed");
            else if (st == 0) {
                *tail_len = tl; *n_pieces = pieces;
                uint64_t at = 0;
                bool ok = true;
                for (int j = 0; j < best_n && ok; ++j) {
                    const aqcgz::OffloadResult& r = res[(size_t)(best0 + j)];
                    ok = off->fetch(r.token, 0, r.n_sym, text + at);
                    at += r.n_sym;
                }
                ok = off->fetch_wait() && ok;
                if (!ok) rc = fail(AQC_ERR_HIP, "gunzip probe: fetch() failed");
                *n_text = at;
            }
        }
    }
    for (auto& r : res) if (r.token) off->release(r.token);
    return rc;
}

}  // extern "C"
