// aqc_pipe.cpp — whole-input pipeline above the per-chunk C ABI (include/afterqc_hip.h): the byte path of
// seqFilter.run's main loop (preprocesser.py:411-631 with fastq.Reader / fastq.Writer around it) without Python in it.
//
//   reader threads (one per input)   file / gzip stream / memory -> page-locked chunk buffers holding EXACTLY
//                                    `chunk_records` records each (the chunk boundary is the 4K-th newline, found with
//                                    per-block newline counts made by the pool thread that fetched the piece); a plain file
//                                    is pread in parallel pieces, a .gz inflated by many threads (aqc_gunzip.cpp)
//   slot workers (per GPU x slots)   chunk pair i -> context i % n_ctx: aqc_frame -> aqc_run -> aqc_qc_stat (first
//                                    qc_sample records only, in chunk order) -> aqc_format -> aqc_fetch_text into
//                                    page-locked output buffers; a worker blocks only on ITS slot's stream, so the
//                                    upload of one chunk, the kernels of another and the download of a third overlap
//   orderer + one writer per file    the chunks' good / bad / overlap streams are committed in chunk order; every output
//                                    file has its own thread issuing large sequential write()s (a file takes ~10 GB/s on the
//                                    MI355X host whatever is done: tools/ubench/io_probe.cpp), .gz as BGZF-compatible
//                                    independent members deflated on the pool (aqc_deflate.cpp)
//
// Records are independent and every statistic is additive (or min-merged by global record index), so one input is
// dealt over any number of GPUs with no collective: chunk i carries first_index = i * chunk_records.
//
// The pipeline handles the REGULAR shape of an input — 4-line records, both mates with the same number of records, no
// empty line inside.  Anything else (fastq.py:44-47's "empty line ends the file", mates of different lengths, ...)
// is detected from the frame info and reported as `anomaly`; the caller then reruns the input through the serial
// chunk loop, which reproduces the reference's reader semantics case by case.
//
// One translation unit, in four files:
//   aqc_pipe_prim.hpp     clocks, the bounded queue, on / off environment knobs
//   aqc_pipe_source.hpp   newline counting and the byte sources (file, bzip2, gzip)
//   aqc_pipe_out.hpp      the output file, the BGZF member, the host buffer
//   aqc_pipe.cpp          this file: the chunks, `struct Run` (one run's queues, locks and thread bodies) and the C ABI
#include <sys/stat.h>
#include <sys/uio.h>
#include <zlib.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/afterqc_hip.h"
#include "aqc_gz.hpp"
#include "aqc_keep.hpp"
#include "aqc_pool.hpp"
#include "aqc_pipe_prim.hpp"
#include "aqc_pipe_source.hpp"
#include "aqc_pipe_out.hpp"

#ifdef AQC_GZ_PROFILE
namespace aqcgz { extern std::atomic<long> gz_prof[6]; }
#endif

namespace {

char g_pipe_err[512] = "";
std::mutex g_pipe_err_mu;

struct InChunk {
    uint64_t idx = 0;
    const uint8_t* data = nullptr;
    uint64_t bytes = 0, lines = 0;
    bool final = false;
    int buf = -1;        // index into the file's buffer ring (-1: zero-copy view of a memory source)
    // stretches of the chunk whose bytes are NOT in `data` but in the memory of the device the chunk is dealt to (a .gz input
    // decoded there: aqc_frame_mixed), sorted by offset; they hold their sections — and so the text — until the chunk is framed
    std::shared_ptr<std::vector<aqcgz::DevSegment>> ext;
    uint8_t last_byte = '\n';
};

struct OutChunk {
    uint64_t idx = 0;
    int set = -1;                // output buffer set (owned by a slot worker)
    int worker = -1;
    uint64_t sizes[6] = {0, 0, 0, 0, 0, 0};
    uint64_t gz_sizes[6] = {0, 0, 0, 0, 0, 0};      // the streams as gzip members made on the device (gz == true)
    bool gz = false;
    uint64_t n = 0;
    bool last = false;
    bool fatal = false;          // upstream's run ends behind this chunk's n records (Run::dies_at_record)
    bool fused = false;          // its records were placed by the verdict kernel (AQC_FUSED=1: aqc_format_fused)
    // plain-text output WITHOUT the copy nobody needs (aqc_format_spans): the good records that go out as their own bytes are
    // written straight from the chunk's input buffer, which therefore lives until the chunk is committed; sizes[0] / sizes[3]
    // are then only the rebuilt good records, good_total what the good files really get
    struct Spans {
        std::vector<aqc_span_event> ev[2];
        const uint8_t* in[2] = {nullptr, nullptr};
        uint64_t end[2] = {0, 0};            // chunk bytes up to the end of record n - 1
        uint64_t good_total[2] = {0, 0};
    };
    std::shared_ptr<Spans> spans;
    int in_buf[2] = {-1, -1};    // input ring buffers this chunk still holds (spans mode), -1: none
    // the good output of file f, put together on the host by the slot worker (spans mode "assemble"): the file writer issues
    // ONE write() of it, as for a stream the device formatted
    const uint8_t* good_ptr[2] = {nullptr, nullptr};
    uint64_t good_bytes[2] = {0, 0};
};

// The good output of one file of a chunk formatted by aqc_format_spans, in order: the chunk's own bytes from the end of one
// event's record to the start of the next (`own(offset in the chunk, length)`, never of length 0), `out_len` rebuilt bytes at
// every event (`patch(length)`, once per event, 0 for a bad record), and the chunk's own bytes behind the last event up to `end`.
// Events [e0, e1) are walked; a walk that does not reach the chunk's tail passes end = 0.
template <class Own, class Patch>
inline void walk_spans(const aqc_span_event* ev, size_t e0, size_t e1, uint64_t end, Own&& own, Patch&& patch) {
    uint64_t cursor = e0 ? (uint64_t)ev[e0 - 1].in_start + ev[e0 - 1].in_len : 0;
    for (size_t i = e0; i < e1; ++i) {
        if (ev[i].in_start > cursor) own(cursor, (uint64_t)ev[i].in_start - cursor);
        patch((uint64_t)ev[i].out_len);
        cursor = (uint64_t)ev[i].in_start + ev[i].in_len;
    }
    if (end > cursor) own(cursor, end - cursor);
}

// Device decoders of .gz and .bz2 inputs outlive the pipe that made them: a decoder that has worked holds gigabytes of device
// buffers and page-locked stages — freeing them took a one-shot CLI run 34 ms of its pass 2 (two decoders, one after the other),
// and a folder of inputs (after.py -d: a pipe per file) would set them up again for every file.  A pipe that is destroyed gives
// its decoders to a keeper (aqc_keep.hpp: never destroyed, nothing is freed at exit()), the next pipe that asks with an equal key
// — the device and everything the decoder was built with — takes them over warm.
struct GzDecoder {
    std::unique_ptr<aqcgz::SectionOffload> dec;
    bool warm = false;       // it has run before: its device buffers and page-locked arenas exist
    bool gave_up() { return dec->gave_up(); }
};
using GzKey = std::pair<int, aqcgz::OffloadOpts>;       // device, options
using Bz2Key = std::pair<int, size_t>;                  // device, blocks per group (aqc_bunzip2_offload.hip)
aqc::Keep<GzKey, GzDecoder>* const g_gz_keep = new aqc::Keep<GzKey, GzDecoder>;
aqc::Keep<Bz2Key, aqcbz::StreamDecoder>* const g_bz2_keep = new aqc::Keep<Bz2Key, aqcbz::StreamDecoder>;

// The decoder of one kind that one input file of a pipe holds: taken from its keeper or made with the first input that wants it
// (Run::take), given back when the pipe is destroyed if it still works.
template <class Key, class T>
struct Held {
    Key key{};
    std::unique_ptr<T> dec;
    bool tried = false;
    // (what comes back from a keeper that is full dies with the pipe)
    void give_back(aqc::Keep<Key, T>* keep) { if (dec && !dec->gave_up()) dec = keep->give(key, std::move(dec)); }
};

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
struct aqc_pipe {
    int n_ctx = 0;
    std::vector<aqc_ctx*> ctx;
    int slots = 2;
    int io_threads = 8;
    std::unique_ptr<Pool> pool;
    // per input file: the device decoder of its gzip stream (with the first .gz input, kept: its device buffers and page-locked
    // arenas are as expensive to set up as a whole run) and of its bzip2 blocks (with the first .bz2 input given to the device)
    struct InputDecoders {
        Held<GzKey, GzDecoder> gz;
        Held<Bz2Key, aqcbz::StreamDecoder> bz2;
    } dec[2];
    // The buffers come last: they are the first thing `delete` frees (aqc_pipe_destroy), ahead of the decoders and the pool.
    // per input file: ring of page-locked chunk buffers
    std::vector<HostBuf> in_buf[2];
    // per worker (ctx, slot): two sets of six output buffers
    struct WorkerBufs { HostBuf out[2][6]; HostBuf good[2][2]; };       // good[set][file]: assembled good output (plain memory)
    std::vector<WorkerBufs> wbufs;
};

namespace {

struct Run {
    // ---- what the run is given ------------------------------------------------------------------------------------------------
    aqc_pipe* P;
    const aqc_pipe_io* io;
    const aqc_pipe_opts* opt;
    aqc_pipe_result* res;
    int nf = 1;
    uint64_t K = 0;
    // ---- what it reads from the environment when it starts (Run::Run; the knobs of a .gz input: open_source) --------------------
    bool dbg = false;                  // AQC_PIPE_DEBUG
    bool spans_on = false;             // plain-text output: good records that go out as their own bytes are not copied on the device (aqc_format_spans) ...
    bool spans_assemble = false;       // ... and the slot worker puts each good file's chunk together on the host (else: the file writers writev the pieces)
    bool gz_on_device = false;
    int io_node = -1;                  // the NUMA node every context's GPU hangs off (-1: they differ, or unknown): readers, the dispatcher, the
                                       // commit thread and the file writers run there too, next to the rings they fill and drain
    // ---- how it ends --------------------------------------------------------------------------------------------------------
    std::atomic<bool> abort{false}, anomaly{false};
    std::mutex err_mu;
    std::string err;
    int err_code = 0;
    // the run ends at a record (dies_at_record): the earliest chunk that says so, and what it said
    uint64_t fatal_chunk = UINT64_MAX;
    std::string fatal_err;
    int fatal_code = 0;

    // ---- readers -> dispatcher: chunks in input buffer rings ------------------------------------------------------------------------
    std::unique_ptr<BQueue<InChunk>> inq[2];
    std::mutex ring_mu[2];
    std::condition_variable ring_cv[2];
    std::vector<char> ring_free[2];

    // ---- dispatcher -> slot workers (one queue per context) -------------------------------------------------------------------------
    struct Job { InChunk c[2]; uint64_t idx; bool last; uint64_t ticket; };
    std::vector<std::unique_ptr<BQueue<Job>>> jobq;
    // DMA gates, one pair per physical device: the uploads (and the downloads) of the chunks dealt to ONE device start in
    // chunk order and at most `slots` of them run at a time.  With one context per GPU that never blocks; with several
    // contexts on one device it keeps a dozen transfers from sharing the link equally and all finishing late, which
    // starves the in-order writers.
    struct Gate {
        std::mutex mu;
        std::condition_variable cv;
        uint64_t started = 0, finished = 0;
    };
    std::vector<std::unique_ptr<Gate>> up_gate, down_gate;
    std::vector<int> group_of_ctx;
    std::vector<uint64_t> group_tickets;

    // ---- among the slot workers, in chunk order: the end of the input, the QC turn ------------------------------------------------------
    // End of input inside the pipe (fastq.py:37-49, preprocesser.py:412-429).  A chunk is RUN only once every chunk before it has been
    // framed and found to continue the input: the chunk in which the input ends (an empty line, a partial last record, a mate file
    // that is shorter) becomes the run's last, chunks behind it are dropped before anything of them reaches a counter.
    std::mutex fr_mu;
    std::condition_variable fr_cv;
    uint64_t framed_next = 0, end_chunk = UINT64_MAX;
    std::atomic<bool> ended{false};        // the input has ended in a chunk: readers and the dispatcher stop feeding
    uint64_t extra_bases = 0;
    // QC turn taking (post-filter sampling must be issued in chunk order, see aqc_qc_stat's time keys)
    std::mutex qc_mu;
    std::condition_variable qc_cv;
    uint64_t qc_next = 0;

    // ---- slot workers -> commit thread: chunks in output buffer sets --------------------------------------------------------------------
    BQueue<OutChunk> outq{0};
    std::mutex set_mu;
    std::condition_variable set_cv;
    std::vector<char> set_free;        // [worker * 2 + set]

    // ---- commit thread -> file writers ----------------------------------------------------------------------------------------------
    // a committed chunk on its way through the per-file writer threads; the last one to finish hands the buffer set back
    struct Commit {
        OutChunk oc;
        std::atomic<int> remaining{0};
    };
    std::unique_ptr<BQueue<std::shared_ptr<Commit>>> fileq[6];
    OutFile out[6];
    // (file, chunk) writes handed to the file writers / finished by them: the run that dies at a record stops the pipe only once
    // EVERY chunk committed before it has reached its files (waiting for the fatal chunk's own files alone let stop_all() cancel
    // earlier chunks still queued on a file the fatal chunk does not write to)
    std::atomic<uint64_t> writes_queued{0}, writes_done{0};
    std::shared_ptr<Commit> fatal_commit;

    // ---- what it reports ------------------------------------------------------------------------------------------------------------
    std::atomic<uint64_t> records{0};
    std::atomic<uint64_t> ns_read{0}, ns_count{0}, ns_frame{0}, ns_kernels{0}, ns_fetch{0}, ns_write{0}, ns_wait_set{0}, ns_wait_ring{0};
    // (AQC_PIPE_DEBUG: CPU seconds per kind of thread, printed at the end — who uses the host's cores)
    std::atomic<long> cpu_us[5] = {{0}, {0}, {0}, {0}, {0}};       // file writers, readers, dispatcher, slot workers, commit thread
    double cpu_proc0 = 0, cpu_pool0 = 0;

    // ---- set-up: queues, ring occupancy, gates by physical device, the I/O threads' node, the modes of the output -----------------------
    // only_file >= 0: the run of ONE reader and nothing else (aqc_pipe_split: a pipe without contexts, `opt` without output)
    Run(aqc_pipe* pipe, const aqc_pipe_io* io_, const aqc_pipe_opts* opt_, aqc_pipe_result* res_, int only_file = -1)
        : P(pipe), io(io_), opt(opt_), res(res_) {
        nf = (only_file < 0 && (io->in_path[1] || io->in_mem[1])) ? 2 : 1;
        K = opt->chunk_records ? opt->chunk_records : (1u << 17);
        dbg = getenv("AQC_PIPE_DEBUG") != nullptr;
        {
            // Plain-text outputs, OPT-IN: the good records that go out as their own bytes never leave the host (aqc_format_spans): no copy
            // on the device (the device step of 10 M reads 4.7 -> 3.2 ms, 17.3 -> 10.7 GB of HBM traffic), no download (3.1 of the
            // 3.44 GB per 10 M reads stay off PCIe: pinned -> pinned 105 -> 122 - 160 Mreads/s).  Two ways to get them into the good files:
            //   AQC_SPANS=1  writev: the file writers writev the pieces straight from the input buffers — no host copy, but a
            //                run of whole records is 3 - 4 KB in the bench workload and an iovec costs the kernel ~60 ns: 9.2 - 9.9 GB/s
            //                against write()'s 11 - 12 on a path bound by exactly those two writers (file -> file 0.18 -> 0.23 s,
            //                profiles/r05_spans_ab.txt);
            //   AQC_SPANS=2  assemble: the slot worker puts each good file's chunk together in host memory — the chunk's own
            //                bytes between the events, the rebuilt records at them, copied on the pool in ~1 MiB tasks — and the file
            //                writer issues one big write() as it always did.  Tried as the DEFAULT and taken back: interleaved on one
            //                box the text step gives 50.2 - 51.4 Mreads/s, this 39.6 - 48.2 (two inputs at once: 72 - 76 against 55 - 68;
            //                the 100 M-read input 19 against 44 - 52; profiles/r06_spans_assemble_ab.txt) — the host copies every
            //                output byte once more, on the 16 granted CPUs that the readers' and the writers' own copies already
            //                share, and the writers then read buffers that pool threads of either socket have just written.
            // So the DEFAULT stays the text step (aqc_format: everything formatted on the device and downloaded): a run is bound by its
            // two file writers, and the text step is what leaves them alone.  Both spans modes pay where PCIe or the device is the
            // bound and the host has cycles to spare.  (.gz output needs the whole text on the device, where its members are built; a
            // .gz input decoded on the device keeps its text in HBM and has no host copy to assemble from.)
            const char* e = getenv("AQC_SPANS");
            spans_on = !io->gzip_out && !opt->no_output && e && (e[0] == '1' || e[0] == '2');
            spans_assemble = spans_on && e[0] == '2';
        }
        // .gz output: the members are made on the device (aqc_gzdev.hpp) and come back compressed — no host CPU for
        // deflate, a third of the bytes over PCIe.  --compression 0 (stored) and AQC_GZ_DEVICE=0 keep the host codec.
        gz_on_device = io->gzip_out && io->gzip_level >= 1 && !opt->no_output && env_on("AQC_GZ_DEVICE");
        for (int f = 0; f < 2; ++f) {
            if (only_file < 0 ? f >= nf : f != only_file) continue;
            inq[f].reset(new BQueue<InChunk>(2));
            // (the whole ring only when chunks keep their input buffers until they are written — spans mode; else one buffer per slot + two:
            //  every buffer used is a buffer page-locked, which a one-shot run pays for)
            const size_t use = (spans_on && !spans_assemble) ? P->in_buf[f].size() : std::min(P->in_buf[f].size(), (size_t)(P->n_ctx * P->slots + 2));
            ring_free[f].assign(P->in_buf[f].size(), 0);
            for (size_t i = 0; i < use; ++i) ring_free[f][i] = 1;
        }
        for (int i = 0; i < P->n_ctx; ++i) jobq.emplace_back(new BQueue<Job>((size_t)P->slots));
        set_free.assign(P->wbufs.size() * 2, 1);
        for (int q = 0; q < 6; ++q) fileq[q].reset(new BQueue<std::shared_ptr<Commit>>(0));
        // contexts on the same physical device share one pair of DMA gates
        std::vector<int> devs;
        for (int i = 0; i < P->n_ctx; ++i) {
            const int dv = aqc_device_index(P->ctx[i]);
            int g = -1;
            for (size_t k = 0; k < devs.size(); ++k) if (devs[k] == dv) g = (int)k;
            if (g < 0) { g = (int)devs.size(); devs.push_back(dv); }
            group_of_ctx.push_back(g);
        }
        for (size_t k = 0; k < devs.size(); ++k) { up_gate.emplace_back(new Gate()); down_gate.emplace_back(new Gate()); }
        group_tickets.assign(devs.size(), 0);
        // one node for the I/O threads when every context's GPU hangs off the same one
        io_node = P->n_ctx > 0 ? aqc_device_numa_node(P->ctx[0]) : -1;
        for (int i = 1; i < P->n_ctx; ++i)
            if (aqc_device_numa_node(P->ctx[i]) != io_node) io_node = -1;
    }

    void bind_io_thread(const char* what) {
        const int bound = aqc_bind_thread_to_node(io_node);
        if (dbg)
            fprintf(stderr, "pipe: %s thread — NUMA node %d, %s\n", what, io_node, bound ? "bound to that node's CPUs" : "not bound (contexts on several nodes, single node, unknown, or AQC_PIPE_NUMA=0)");
    }

    // ---- ending the run ---------------------------------------------------------------------------------------------------------
    void fail(int code, const char* fmt, ...) {
        char buf[400];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        {
            std::lock_guard<std::mutex> g(err_mu);
            if (err.empty()) { err = buf; err_code = code; }
        }
        stop_all();
    }
    // the failures several stages share (false: so that a stage can `return no_memory(n);`)
    bool no_memory(size_t n) { fail(AQC_ERR_HIP, "page-locked allocation of %zu bytes failed", n); return false; }
    bool device_copy_failed(int f) { fail(AQC_ERR_HIP, "%s: copying decoded text from the device failed", io->in_path[f]); return false; }
    void close_input() {
        for (int f = 0; f < 2; ++f) {
            if (inq[f]) inq[f]->close();
            ring_cv[f].notify_all();
        }
    }
    void end_input() {
        ended = true;
        close_input();
    }
    void stop_all() {
        abort = true;
        close_input();
        for (auto& q : jobq) q->close();
        outq.close();
        for (int q = 0; q < 6; ++q) if (fileq[q]) fileq[q]->close();
        set_cv.notify_all();
        qc_cv.notify_all();
        fr_cv.notify_all();
        for (auto& g : up_gate) { std::lock_guard<std::mutex> lk(g->mu); g->cv.notify_all(); }
        for (auto& g : down_gate) { std::lock_guard<std::mutex> lk(g->mu); g->cv.notify_all(); }
    }

    // ---- input buffer rings -----------------------------------------------------------------------------------------------------
    int acquire_ring(int f) {
        std::unique_lock<std::mutex> lk(ring_mu[f]);
        int got = -1;
        ring_cv[f].wait(lk, [&] {
            if (abort || ended) return true;
            for (size_t i = 0; i < ring_free[f].size(); ++i)
                if (ring_free[f][i]) { got = (int)i; return true; }
            return false;
        });
        if (abort || ended || got < 0) return -1;
        ring_free[f][got] = 0;
        return got;
    }
    void release_ring(int f, int i) {
        if (i < 0) return;
        {
            std::lock_guard<std::mutex> g(ring_mu[f]);
            ring_free[f][i] = 1;
        }
        ring_cv[f].notify_all();
    }
    // A ring buffer in one owner's hands: it goes back to the ring when the owner is done with it — on every way out — unless it
    // has been handed on (to the chunk that travels on with it).  i < 0: none (a zero-copy chunk of a memory source).
    struct RingHold {
        Run& r;
        const int f;
        int i;
        RingHold(Run& run, int file, int index = -1) : r(run), f(file), i(index) {}
        RingHold(const RingHold&) = delete;
        RingHold& operator=(const RingHold&) = delete;
        ~RingHold() { release(); }
        void release() { r.release_ring(f, i); i = -1; }
        int hand_on() { const int k = i; i = -1; return k; }
        explicit operator bool() const { return i >= 0; }
        HostBuf& buf() const { return r.P->in_buf[f][(size_t)i]; }
    };

    // ---- DMA gates ----------------------------------------------------------------------------------------------------------------
    // A turn at a gate: entered in ticket order, left when the pass goes out of scope (or earlier: leave()).
    struct GatePass {
        Run& r;
        Gate* g = nullptr;
        explicit GatePass(Run& run) : r(run) {}
        GatePass(const GatePass&) = delete;
        GatePass& operator=(const GatePass&) = delete;
        ~GatePass() { leave(); }
        bool held() const { return g != nullptr; }
        bool enter(Gate& gate, uint64_t ticket) {      // false: the run is stopping
            std::unique_lock<std::mutex> lk(gate.mu);
            gate.cv.wait(lk, [&] { return r.abort.load() || (gate.started == ticket && ticket < gate.finished + (uint64_t)r.P->slots); });
            if (r.abort) return false;
            gate.started++;
            g = &gate;
            return true;
        }
        void leave() {
            if (!g) return;
            {
                std::lock_guard<std::mutex> lk(g->mu);
                g->finished++;
            }
            g->cv.notify_all();
            g = nullptr;
        }
    };

    // ---- output buffer sets: a slot worker fills one while the files drain its other ------------------------------------------------------
    bool acquire_set(int wid, int set) {      // waits for the writers to hand the set back; false: the run is stopping
        std::unique_lock<std::mutex> lk(set_mu);
        set_cv.wait(lk, [&] { return abort || set_free[wid * 2 + set]; });
        if (abort) return false;
        set_free[wid * 2 + set] = 0;
        return true;
    }
    void release_set(const OutChunk& oc) {
        for (int f = 0; f < 2; ++f) release_ring(f, oc.in_buf[f]);       // (spans mode: the chunk's input buffers were its good records)
        if (oc.set < 0) return;
        {
            std::lock_guard<std::mutex> g(set_mu);
            set_free[oc.worker * 2 + oc.set] = 1;
        }
        set_cv.notify_all();
    }

    // ---- readers: chunks of exactly K records ---------------------------------------------------------------------------------------
    // Three of them — over memory, over a byte source into ring buffers, over a .gz whose device-decoded text stays in HBM — which
    // differ in how they count line feeds.  What a chunk's buffer holds at first, how it grows and how a chunk is closed is the same.
    size_t estimate(double est, size_t slack) const { return (size_t)(est * 1.02 * (double)K) + slack; }      // bytes of K records of `est` bytes
    // the next ring buffer of file f, with room for the estimate (and for what the last chunk left behind its cut); false: the reader ends
    bool open_chunk(RingHold& rb, double est, size_t carried, size_t& cap) {
        const uint64_t tw = now_ns();
        rb.i = acquire_ring(rb.f);
        ns_wait_ring += now_ns() - tw;
        if (!rb) return false;
        cap = estimate(est, 256 << 10);
        if (cap < carried + (1 << 20)) cap = carried + (1 << 20);
        rb.buf().ensure(cap);
        return rb.buf().p ? true : no_memory(cap);
    }
    // the records are longer than estimated: a bigger buffer, keep what is there
    bool grow_chunk(HostBuf& hb, size_t& cap, size_t fill) {
        const size_t ncap = cap + cap / 2 + (4 << 20);
        if (!hb.grow(ncap, fill)) return no_memory(ncap);
        cap = ncap;
        return true;
    }
    // The chunk is cut (idx, data, bytes are set): `lines` line feeds were seen up to the cut or the end, `final` says that nothing
    // of the input is left.  Counts the unterminated last line, refines the estimate, passes the chunk — and its ring buffer — on.
    // false: the reader's loop ends (this was the last chunk, or nobody takes chunks any more).
    bool close_chunk(InChunk& c, RingHold& rb, uint64_t lines, bool final, uint8_t last_byte, double& est) {
        const uint64_t want_lines = 4 * K;
        c.lines = std::min<uint64_t>(lines, want_lines);
        c.final = final;
        if (final && c.bytes > 0 && last_byte != '\n' && lines < want_lines) c.lines += 1;     // unterminated last line
        if (c.lines >= 4 && c.bytes) est = (double)c.bytes / (double)(c.lines / 4);
        c.buf = rb.i;
        if (!inq[rb.f]->push(c)) return false;
        rb.hand_on();
        return !final;
    }

    void reader(int f) {
        bind_io_thread(f == 0 ? "reader (file 1)" : "reader (file 2)");     // (the ring buffers it allocates are first touched here)
        if (io->in_mem[f]) { read_memory(f); return; }
        GzSource* stretches = nullptr;
        std::unique_ptr<Source> src = open_source(f, &stretches);
        if (!src) return;
        if (stretches) read_stretches(f, stretches, file_device(f));
        else read_source(f, *src);
    }

    // The byte source of input file f (nullptr: there is none — the run has been stopped).  *stretches: it is a .gz the device decodes
    // and whose text is to stay there (read_stretches).
    std::unique_ptr<Source> open_source(int f, GzSource** stretches) {
        std::unique_ptr<Source> src;
        if (io->gzip_in[f] == 2) {
            if (!Bz2Api::get().ok) {
                // no libbz2 to load: not an error of the input — the caller's serial loop reads .bz2 through python's own module
                anomaly = true;
                stop_all();
                return nullptr;
            }
            // bzip2 input: a big stream's blocks go to the device of context f % n in groups.  OPT-IN (AQC_BZ2_DEVICE_IN=1) for
            // streams of more than 8 MiB compressed; AQC_BZ2_DEVICE_MIN=<bytes> moves that limit (below 8 MiB: a test hook).  No
            // cold limit is set here: the CLI table it has to come from (tools/gpu_bunzip2_dev.py) has not been measured yet —
            // DESIGN.md §4.4.  AQC_BZ2_DEVICE_IN=0, no context, a smaller stream, a pbzip2-style file of many small streams:
            // libbz2 alone, as before.
            size_t bz_min = (size_t)(8u << 20) + 1;
            if (const char* m = getenv("AQC_BZ2_DEVICE_MIN")) bz_min = (size_t)std::max(0ll, atoll(m));
            const char* bz_in = getenv("AQC_BZ2_DEVICE_IN");
            struct stat bst;
            aqcbz::StreamDecoder* bz_dec = nullptr;
            if (bz_in && bz_in[0] == '1' && !P->ctx.empty() && stat(io->in_path[f], &bst) == 0 && (size_t)bst.st_size >= bz_min) {
                // (the pipe's own from an earlier run while it works, else a kept or a new one)
                auto& h = P->dec[f].bz2;
                if (!h.dec || h.dec->gave_up()) take(f, "bunzip2", g_bz2_keep, h, Bz2Key(file_device(f), 0), [&] { return aqcbz::make_device_bunzip2(h.key.first, h.key.second); });
                bz_dec = h.dec.get();
            }
            src.reset(new Bz2Source(io->in_path[f], P->pool.get(), bz_dec, bz_min));
        } else if (io->gzip_in[f]) {
            // gzip input: the GPUs take groups of sections off the pool's hands (file f -> the device of context f % n)
            const bool device_in = env_on("AQC_GZ_DEVICE_IN");
            auto& h = P->dec[f].gz;
            if (device_in && !h.tried && !P->ctx.empty()) {      // (set up with the first .gz input of this file slot)
                size_t group = 96u << 20;       // (measured, warm pipe, 0.59 GB inputs: groups of 16 / 32 / 96 MiB = 34 / 38 / 42.5 Mreads/s — profiles/r06_gz_hbm_ab.txt)
                if (const char* g = getenv("AQC_GZ_GROUP")) group = (size_t)std::max(1ll, atoll(g));
                take(f, "gunzip", g_gz_keep, h, GzKey(file_device(f), aqcgz::offload_opts(group)), [&]() -> GzDecoder* {
                    aqcgz::SectionOffload* d = aqcgz::make_device_offload(h.key.first, h.key.second);
                    return d ? new GzDecoder{std::unique_ptr<aqcgz::SectionOffload>(d)} : nullptr;
                });
            }
            // Which files the device is asked for.  A cold decoder — buffers by need (2 - 3 GB for groups of 62 MiB), set up in the
            // background while the pool keeps every section (SectionOffload::prepare), markers + CRC-32 resolved on the device — is
            // started for every input of >= 448 MiB compressed (about 8 M reads).  Measured through the CLI, a fresh process per
            // run (profiles/r06_gz_cold_cli.txt): 10 M reads in two files of 0.59 GB — pass 2 0.37 - 0.41 s with the device,
            // 0.40 - 0.47 s with the pool alone; 4 M reads of the config-5 flavour in two files of 0.36 GB — 0.41 against 0.33 s:
            // a run of a quarter of a second is over before the decoder has paid for its set-up.  A warm one — the pipe object has
            // decoded a .gz input of this slot with it before: a service, a folder of files, bench.py — for everything the pool
            // would need longer for than a group takes the device (48 MiB).  AQC_GZ_DEVICE_MIN=<bytes> sets the limit for both.
            // (How the limit came down from 4 GiB: DESIGN.md §4, profiles/r05_gz_cold_decoder.txt.)
            size_t dev_min = h.dec && h.dec->warm ? (size_t)(48u << 20) : (size_t)(448u << 20);
            if (const char* m = getenv("AQC_GZ_DEVICE_MIN")) dev_min = (size_t)std::max(0ll, atoll(m));
            struct stat gst;
            const bool use_dev = device_in && h.dec && stat(io->in_path[f], &gst) == 0 && (size_t)gst.st_size >= dev_min;
            if (use_dev) h.dec->warm = true;
            GzSource* gs = new GzSource(io->in_path[f], P->pool.get(), 0, use_dev ? h.dec->dec.get() : nullptr);
            src.reset(gs);
            // the text of the sections the device decodes stays in HBM and is framed from there — for the chunks that are dealt
            // to the decoder's own device, with plain chunk buffers (the spans mode writes good records FROM them)
            if (use_dev && !gs->failed() && gs->takes_segments() && !spans_on && env_on("AQC_GZ_HBM")) { *stretches = gs; return src; }
        } else src.reset(new FileSource(io->in_path[f], P->pool.get()));
        if (src->failed()) { fail(AQC_ERR_ARG, "cannot open %s", io->in_path[f]); return nullptr; }
        return src;
    }
    int file_device(int f) const { return aqc_device_index(P->ctx[(size_t)f % P->ctx.size()]); }
    // a decoder for input file f: the one that waits in the keeper under `key`, left there by an earlier pipe, or a new one
    // (null: it cannot be made — nobody asks again)
    template <class Key, class T, class Make>
    void take(int f, const char* kind, aqc::Keep<Key, T>* keep, Held<Key, T>& h, const Key& key, Make&& make) {
        h.tried = true;
        h.key = key;
        h.dec = keep->take(key);
        if (dbg) fprintf(stderr, "pipe: input %d takes its %s decoder on device %d: %s\n", f, kind, key.first, h.dec ? "warm from the keeper" : "new");
        if (!h.dec) h.dec.reset(make());
    }

    // host memory: zero-copy chunks, counted over a span that grows until it holds K records
    void read_memory(int f) {
        const uint64_t want_lines = 4 * K, total = io->in_mem_bytes[f];
        double est = 360.0;                 // bytes per record, refined after the first chunk
        uint64_t mpos = 0;
        for (uint64_t idx = 0; !abort; ++idx) {
            const uint8_t* base = io->in_mem[f] + mpos;
            const uint64_t left = total - mpos;
            uint64_t span = std::min<uint64_t>(left, estimate(est, 64 << 10));
            std::vector<uint32_t> cnt;
            uint64_t lines = 0;
            for (;;) {
                const size_t b0 = cnt.size(), b1 = (size_t)((span + SUB - 1) / SUB);
                cnt.resize(b1);
                P->pool->parallel_for(b1 - b0, [&](size_t i) {
                    const size_t o = (b0 + i) * SUB;
                    cnt[b0 + i] = (uint32_t)count_nl(base + o, (size_t)std::min<uint64_t>(SUB, span - o));
                });
                lines = 0;
                for (auto v : cnt) lines += v;
                if (lines >= want_lines || span == left) break;
                const uint64_t nspan = std::min<uint64_t>(left, span + span / 2 + (1 << 20));
                // recount the (partial) last block of the old span together with the new bytes
                if (!cnt.empty()) cnt.pop_back();
                span = nspan;
            }
            InChunk c;
            c.idx = idx;
            c.data = base;
            c.bytes = lines >= want_lines ? locate_nl(base, (size_t)span, cnt, want_lines) : span;
            mpos += c.bytes;
            RingHold none(*this, f);
            if (!close_chunk(c, none, lines, mpos == total, c.bytes ? base[c.bytes - 1] : (uint8_t)'\n', est)) break;
        }
        inq[f]->close();
    }

    // a byte source: into ring buffers, counted per block by the thread that fetched the piece (Source::read_counted)
    void read_source(int f, Source& src) {
        const uint64_t want_lines = 4 * K;
        double est = 360.0;                 // bytes per record, refined after the first chunk
        std::vector<uint8_t> carry;
        bool eof = false;
        for (uint64_t idx = 0; !abort; ++idx) {
            RingHold rb(*this, f);
            size_t cap = 0;
            if (!open_chunk(rb, est, carry.size(), cap)) return;
            HostBuf& hb = rb.buf();
            size_t fill = carry.size();
            if (fill) memcpy(hb.p, carry.data(), fill);
            carry.clear();
            std::vector<uint32_t> cnt;
            uint64_t lines = 0;
            if (fill) Source::count_blocks(hb.p, 0, fill, cnt, P->pool.get());      // the carried-over bytes
            for (;;) {
                if (!eof && fill < hb.cap) {
                    const size_t want = std::min(hb.cap, cap) - fill;
                    const uint64_t tr = now_ns();
                    // (bytes and their per-block newline counts in one go: the thread that fetched a piece counts it)
                    const size_t got = want ? src.read_counted(hb.p, fill, want, cnt, P->pool.get()) : 0;
                    ns_read += now_ns() - tr;
                    if (src.failed()) { fail(AQC_ERR_ARG, "%s: %s", io->in_path[f], src.why()); return; }
                    if (got < want) eof = true;
                    fill += got;
                }
                lines = 0;
                for (auto v : cnt) lines += v;
                if (lines >= want_lines || eof) break;
                if (!grow_chunk(hb, cap, fill)) return;
            }
            InChunk c;
            c.idx = idx;
            c.data = hb.p;
            c.bytes = lines >= want_lines ? locate_nl(hb.p, fill, cnt, want_lines) : fill;
            if (c.bytes < fill) carry.assign(hb.p + c.bytes, hb.p + fill);
            if (!close_chunk(c, rb, lines, eof && carry.empty(), c.bytes ? hb.p[c.bytes - 1] : (uint8_t)'\n', est)) break;
        }
        inq[f]->close();
    }

    // ---- reader of a .gz input whose device-decoded text stays in HBM ------------------------------------------------------------
    // The same chunks of exactly K records, but a chunk under construction is a list of STRETCHES: host bytes (what the pool decoded,
    // in the ring buffer) and device text (resolved sections of the device decoder, aqcgz::DevSegment: their place in the ring
    // buffer stays unwritten).  Line feeds: host stretches are counted here, device stretches come with a count per 64 KiB piece
    // from the kernel that checksummed them (gzb_crc_kernel); the <= 2 pieces a stretch covers only partly, and the piece the
    // chunk is cut in, are copied down (64 KiB each) and looked at here.  The text itself crosses PCIe only for chunks that go to
    // ANOTHER device than the decoder's (fetched into the ring buffer).
    struct Stretch {
        size_t off = 0, len = 0;          // in the chunk buffer
        uint64_t nl = 0;
        bool dev = false;
        aqcgz::DevSegment d;              // dev: d.sec_off / d.len follow off / len when the stretch is cut
    };
    // line feeds of host memory, on the pool when it is worth it
    uint64_t count_host(const uint8_t* p, size_t n) {
        if (n < 4 * SUB) return count_nl(p, n);
        const size_t nb = (n + SUB - 1) / SUB;
        std::vector<uint32_t> c(nb);
        P->pool->parallel_for(nb, [&](size_t i) { c[i] = (uint32_t)count_nl(p + i * SUB, std::min(SUB, n - i * SUB)); });
        uint64_t t = 0;
        for (auto v : c) t += v;
        return t;
    }
    // piece j of a section of n bytes: [lo, hi)
    static void piece_range(size_t n, size_t j, size_t& lo, size_t& hi) {
        const size_t pieces = (n + aqcgz::NL_PIECE - 1) / aqcgz::NL_PIECE;
        hi = n - (pieces - 1 - j) * aqcgz::NL_PIECE;
        lo = hi > aqcgz::NL_PIECE ? hi - aqcgz::NL_PIECE : 0;
    }
    static size_t piece_of(size_t n, size_t pos) {      // the piece byte `pos` of a section of n bytes lies in
        const size_t pieces = (n + aqcgz::NL_PIECE - 1) / aqcgz::NL_PIECE;
        const size_t from_end = (n - 1 - pos) / aqcgz::NL_PIECE;
        return pieces - 1 - from_end;
    }
    // bytes [a, b) of the section behind a device stretch -> host memory `to` (synchronous: a piece at most)
    static bool fetch_now(const aqcgz::DevSegment& d, size_t a, size_t b, uint8_t* to) {
        return b <= a || (d.owner->fetch(d.token, a, b - a, to) && d.owner->fetch_wait());
    }
    // line feeds of a device stretch: whole pieces from the decoder's counts, partly covered ones copied down (into `tmp`)
    bool count_dev(const aqcgz::DevSegment& d, uint64_t& nl, std::vector<uint8_t>& tmp) {
        nl = 0;
        if (!d.len) return true;
        const size_t a = d.sec_off, b = d.sec_off + d.len;
        for (size_t j = piece_of(d.sec_len, a), j1 = piece_of(d.sec_len, b - 1); j <= j1; ++j) {
            size_t lo, hi;
            piece_range(d.sec_len, j, lo, hi);
            if (lo >= a && hi <= b) { nl += d.piece_nl[j]; continue; }
            const size_t x = std::max(lo, a), y = std::min(hi, b);
            tmp.resize(aqcgz::NL_PIECE);
            if (!fetch_now(d, x, y, tmp.data())) return false;
            nl += count_nl(tmp.data(), y - x);
        }
        return true;
    }
    // offset, inside a device stretch, just behind its `want`-th line feed (1 <= want <= its count)
    bool locate_dev(const aqcgz::DevSegment& d, uint64_t want, size_t& pos, std::vector<uint8_t>& tmp) {
        const size_t a = d.sec_off, b = d.sec_off + d.len;
        uint64_t seen = 0;
        for (size_t j = piece_of(d.sec_len, a), j1 = piece_of(d.sec_len, b - 1); j <= j1; ++j) {
            size_t lo, hi;
            piece_range(d.sec_len, j, lo, hi);
            const size_t x = std::max(lo, a), y = std::min(hi, b);
            const bool whole = lo >= a && hi <= b;
            if (whole && seen + d.piece_nl[j] < want) { seen += d.piece_nl[j]; continue; }
            tmp.resize(aqcgz::NL_PIECE);
            if (!fetch_now(d, x, y, tmp.data())) return false;
            for (size_t i = 0; i < y - x;) {
                const uint8_t* q = (const uint8_t*)memchr(tmp.data() + i, '\n', y - x - i);
                if (!q) break;
                i = (size_t)(q - tmp.data()) + 1;
                if (++seen == want) { pos = x + i - a; return true; }
            }
        }
        return false;       // (counts and bytes disagree: cannot happen)
    }

    // the chunk this reader is putting together, and what the one before left behind its cut
    struct StretchChunk {
        int f = 0;
        std::vector<Stretch> st;               // the chunk so far
        size_t fill = 0;                       // bytes of the ring buffer they cover
        uint64_t lines = 0;                    // line feeds in them
        std::vector<Stretch> carry;            // what the previous chunk left behind its cut (offsets from 0)
        std::vector<uint8_t> carry_host, tmp;  // ... the host bytes of it (carry_host.size() = its whole length; device stretches' places unwritten)
    };
    // the chunk starts with what the last one left behind its cut
    bool take_carry(StretchChunk& k, HostBuf& hb, bool same_dev) {
        k.st.clear();
        k.fill = k.carry_host.size();
        k.lines = 0;
        if (k.fill) memcpy(hb.p, k.carry_host.data(), k.fill);
        for (Stretch& c : k.carry) {
            if (c.dev && !same_dev) {
                // (this chunk goes to another device: its device text comes down after all)
                if (!fetch_now(c.d, c.d.sec_off, c.d.sec_off + c.d.len, hb.p + c.off)) return device_copy_failed(k.f);
                c.dev = false;
                c.d = aqcgz::DevSegment();
            }
            k.lines += c.nl;
            k.st.push_back(std::move(c));
        }
        k.carry.clear();
        k.carry_host.clear();
        return true;
    }
    // `got` new bytes behind k.fill as stretches: the device segments among them, host bytes between them
    bool add_stretches(StretchChunk& k, HostBuf& hb, size_t got, std::vector<aqcgz::DevSegment>& segs) {
        const uint64_t tc = now_ns();
        size_t cur = 0;
        auto host_part = [&](size_t a, size_t b) {
            if (b <= a) return;
            Stretch h;
            h.off = k.fill + a; h.len = b - a;
            h.nl = count_host(hb.p + h.off, h.len);
            k.lines += h.nl;
            k.st.push_back(std::move(h));
        };
        for (aqcgz::DevSegment& g : segs) {
            host_part(cur, g.dst_off);
            Stretch d;
            d.off = k.fill + g.dst_off; d.len = g.len; d.dev = true;
            cur = g.dst_off + g.len;
            d.d = std::move(g);
            if (!count_dev(d.d, d.nl, k.tmp)) return device_copy_failed(k.f);
            k.lines += d.nl;
            k.st.push_back(std::move(d));
        }
        host_part(cur, got);
        ns_count += now_ns() - tc;
        k.fill += got;
        return true;
    }
    // the cut, just behind the 4K-th line feed (k.lines >= 4K): *bytes is where; what lies behind it becomes the carry
    bool cut_stretches(StretchChunk& k, HostBuf& hb, size_t& bytes) {
        const uint64_t want_lines = 4 * K;
        uint64_t seen = 0;
        for (size_t i = 0; i < k.st.size(); ++i) {
            Stretch& x = k.st[i];
            if (seen + x.nl < want_lines) { seen += x.nl; continue; }
            size_t pos = 0;      // inside the stretch, behind the line feed
            const uint64_t n = want_lines - seen;
            if (x.dev) {
                if (!locate_dev(x.d, n, pos, k.tmp)) return device_copy_failed(k.f);
            } else {
                uint64_t c = 0;
                const uint8_t* p = hb.p + x.off;
                size_t o = 0;
                while (o < x.len) {
                    const uint8_t* q = (const uint8_t*)memchr(p + o, '\n', x.len - o);
                    if (!q) break;
                    o = (size_t)(q - p) + 1;
                    if (++c == n) break;
                }
                pos = o;
            }
            bytes = x.off + pos;
            // what lies behind the cut is the head of the next chunk
            if (pos < x.len) {
                Stretch t = x;             // (a copy: its DevSegment holds the section too)
                t.off = 0; t.len = x.len - pos; t.nl = x.nl - n;
                if (t.dev) { t.d.sec_off += pos; t.d.len = t.len; t.d.dev += pos; t.d.dst_off = 0; }
                k.carry.push_back(std::move(t));
                x.len = pos; x.nl = n;
                if (x.dev) x.d.len = pos;
            }
            for (size_t j = i + 1; j < k.st.size(); ++j) {
                Stretch t = std::move(k.st[j]);
                t.off -= bytes;
                k.carry.push_back(std::move(t));
            }
            k.st.resize(i + 1);
            break;
        }
        if (bytes < k.fill) k.carry_host.assign(hb.p + bytes, hb.p + k.fill);
        return true;
    }

    void read_stretches(int f, GzSource* src, int dec_device) {
        const uint64_t want_lines = 4 * K;
        double est = 360.0;
        StretchChunk k;
        k.f = f;
        bool eof = false;
        for (uint64_t idx = 0; !abort; ++idx) {
            // chunk idx goes to context idx % n: only there may its device text stay where it is
            const bool same_dev = aqc_device_index(P->ctx[(size_t)(idx % jobq.size())]) == dec_device;
            RingHold rb(*this, f);
            size_t cap = 0;
            if (!open_chunk(rb, est, k.carry_host.size(), cap)) return;
            HostBuf& hb = rb.buf();
            if (!take_carry(k, hb, same_dev)) return;
            while (k.lines < want_lines && !eof) {
                if (k.fill >= cap && !grow_chunk(hb, cap, k.fill)) return;
                const size_t want = std::min(hb.cap, cap) - k.fill;
                std::vector<aqcgz::DevSegment> segs;
                const uint64_t tr = now_ns();
                const size_t got = src->read_segments(hb.p + k.fill, want, same_dev ? &segs : nullptr);
                ns_read += now_ns() - tr;
                if (src->failed()) { fail(AQC_ERR_ARG, "%s: %s", io->in_path[f], src->why()); return; }
                if (got < want) eof = true;
                if (!add_stretches(k, hb, got, segs)) return;
            }
            size_t bytes = k.fill;
            if (k.lines >= want_lines && !cut_stretches(k, hb, bytes)) return;
            InChunk c;
            c.idx = idx;
            c.data = hb.p;
            c.bytes = bytes;
            // the chunk's last byte (the framing wants it on the host), and its device stretches for aqc_frame_mixed
            uint8_t last_byte = '\n';
            if (bytes) {
                const Stretch& z = k.st.back();
                if (!z.dev) last_byte = hb.p[bytes - 1];
                else if (k.lines < want_lines && !fetch_now(z.d, z.d.sec_off + z.d.len - 1, z.d.sec_off + z.d.len, &last_byte)) {      // (cut behind a line feed otherwise)
                    device_copy_failed(f);
                    return;
                }
            }
            c.last_byte = last_byte;
            for (Stretch& x : k.st)
                if (x.dev && x.len) {
                    if (!c.ext) c.ext = std::make_shared<std::vector<aqcgz::DevSegment>>();
                    x.d.dst_off = x.off;
                    c.ext->push_back(std::move(x.d));
                }
            if (!close_chunk(c, rb, k.lines, eof && k.carry.empty() && k.carry_host.empty(), last_byte, est)) break;
        }
        inq[f]->close();
    }

    // ---- dispatcher: pair the chunks, deal them round robin ---------------------------------------------------------------
    void release_inputs(const Job& j) { for (int f = 0; f < nf; ++f) release_ring(f, j.c[f].buf); }
    void dispatcher() {
        bind_io_thread("dispatcher");
        static const uint8_t nothing[1] = {0};
        bool over[2] = {false, nf < 2};       // the file's final chunk has been dealt (a shorter mate: its partner goes on against nothing)
        for (uint64_t idx = 0; !abort && !ended; ++idx) {
            Job j;
            j.idx = idx;
            bool got[2] = {false, false};
            for (int f = 0; f < nf; ++f) {
                if (!over[f]) got[f] = inq[f]->pop(j.c[f]);
                if (!got[f]) {
                    // nothing more of this file: an empty final chunk (upstream's reader returns None from here on)
                    j.c[f] = InChunk();
                    j.c[f].idx = idx; j.c[f].data = nothing; j.c[f].final = true;
                    over[f] = true;
                } else if (j.c[f].final) over[f] = true;
            }
            if (!got[0] && !(nf == 2 && got[1])) break;            // both ran dry (or the pipe is stopping)
            if (abort || ended) { release_inputs(j); break; }
            // (R1's final chunk ends the loop whatever R2 holds: preprocesser.py:412-415)
            j.last = j.c[0].final;
            j.ticket = group_tickets[group_of_ctx[idx % jobq.size()]]++;
            if (!jobq[idx % jobq.size()]->push(j)) { release_inputs(j); break; }
            if (j.last) break;
        }
        for (auto& q : jobq) q->close();
    }

    // ---- slot worker ------------------------------------------------------------------------------------------------------
    // One chunk pair in a slot worker's hands.  It owns the chunk's input buffers: they go back to their rings when the text has
    // left them, or when the worker lets go of the chunk on any other way — unless the chunk's good records are going to be
    // written from them (spans mode), in which case they are handed on to its OutChunk.
    struct Turn {
        aqc_ctx* c;
        int ci, slot, wid;
        Job& j;
        RingHold in[2];
        aqc_text_chunk ch{};
        aqc_frame_info info{};
        uint64_t n = 0;           // records of the chunk that are run and written (info.n, fewer when upstream dies at one)
        bool fatal = false;       // upstream's run ends inside this chunk (an exception in its loop): records [0, n) are written, then the pipe stops
        uint64_t tt = 0;          // since when the stage being timed runs
        Turn(Run& r, aqc_ctx* ctx, int ci_, int slot_, Job& job)
            : c(ctx), ci(ci_), slot(slot_), wid(ci_ * r.P->slots + slot_), j(job), in{{r, 0, job.c[0].buf}, {r, 1, job.c[1].buf}} {}
        void drop_input() { in[0].release(); in[1].release(); }
    };
    enum class Step { go, skip, quit };      // on with this chunk / on with the next one / the worker ends

    void worker(int ci, int slot) {
        aqc_ctx* c = P->ctx[ci];
        // this thread drives one GPU: it runs on the CPUs next to that GPU, and the page-locked output sets it touches first
        // (P->wbufs[wid]) come from that node's memory.  Readers and file writers serve every context: they float.
        {
            const int node = aqc_device_numa_node(c), bound = aqc_bind_thread_to_node(node);
            if (slot == 0 && dbg)
                fprintf(stderr, "pipe: context %d (device %d) — NUMA node %d, its %d slot workers %s; reader / writer / pool threads are not bound (they serve all contexts)\n",
                        ci, aqc_device_index(c), node, P->slots, bound ? "bound to that node's CPUs" : "not bound (single node, unknown, or AQC_PIPE_NUMA=0)");
        }
        Job j;
        int set = 0;
        while (!abort && jobq[ci]->pop(j)) {
            Turn t(*this, c, ci, slot, j);
            if (!frame_chunk(t)) return;
            const Step s = end_of_input(t);
            if (s == Step::quit) return;
            if (s == Step::skip) continue;          // the input ended before this chunk
            OutChunk oc;
            oc.idx = j.idx; oc.last = j.last; oc.worker = t.wid;
            if (t.n == 0) {
                // the input ended at this chunk's very first record (a mate file that ran dry at a chunk boundary, a partial record):
                // nothing to run or to write, but the chunk is committed — it is the run's last
                t.drop_input();
                if (!outq.push(oc)) return;
                continue;
            }
            if (int rc = aqc_run(c, slot, UINT64_MAX)) { fail(rc, "aqc_run: %s", aqc_last_error()); return; }
            if (!qc_turn(t)) return;
            if (!opt->no_output) {
                if (!format_and_fetch(t, oc, set)) return;
                oc.set = set;
                set ^= 1;
            } else if (!sync_only(t)) return;
            oc.n = t.n;
            oc.fatal = t.fatal;
            if (t.fatal) oc.last = true;
            records += t.n;
            if (!outq.push(oc) || t.fatal) return;
        }
    }

    // framing (of host text, or of host text mixed with text in this device's memory) under the upload gate
    bool frame_chunk(Turn& t) {
        Job& j = t.j;
        aqc_text_chunk& ch = t.ch;
        ch.text1 = j.c[0].data; ch.bytes1 = j.c[0].bytes; ch.final1 = j.c[0].final ? 1 : 0;
        if (nf == 2) { ch.text2 = j.c[1].data; ch.bytes2 = j.c[1].bytes; ch.final2 = j.c[1].final ? 1 : 0; }
        ch.max_records = UINT64_MAX;
        ch.first_index = (opt->chunk_index0 + j.idx * (opt->chunk_index_stride ? opt->chunk_index_stride : 1)) * K;
        t.tt = now_ns();
        int rc;
        {
            GatePass up(*this);
            if (!up.enter(*up_gate[group_of_ctx[t.ci]], j.ticket)) return false;
            if (j.c[0].ext || (nf == 2 && j.c[1].ext)) {
                // parts of the chunk are text in this device's memory (a .gz input decoded here): they move inside HBM
                std::vector<aqc_text_extent> ex[2];
                for (int f = 0; f < nf; ++f)
                    if (j.c[f].ext)
                        for (const aqcgz::DevSegment& g : *j.c[f].ext) ex[f].push_back(aqc_text_extent{(uint64_t)g.dst_off, (uint64_t)g.len, g.dev});
                rc = aqc_frame_mixed(t.c, t.slot, &ch, ex[0].data(), ex[0].size(), j.c[0].last_byte, ex[1].data(), ex[1].size(), nf == 2 ? j.c[1].last_byte : (uint8_t)'\n', &t.info);
                for (int f = 0; f < nf; ++f) j.c[f].ext.reset();        // (the sections — and their text — are free to go)
            } else rc = aqc_frame(t.c, t.slot, &ch, &t.info);
        }
        ns_frame += now_ns() - t.tt;
        t.tt = now_ns();
        // the text has left the host buffers — which are free again, unless the good records are going to be written from
        // them (spans mode: they are released when the chunk has been committed)
        if (!spans_on || rc) t.drop_input();
        if (rc) { fail(rc, "aqc_frame: %s", aqc_last_error()); return false; }
        t.n = t.info.n;
        return true;
    }

    // Does the input end in this chunk?  The lock step of preprocesser.py:412-429 over what the framing found: R1 is read
    // first; a reader is dry when its chunk ended (an empty line: eof, or the file's last chunk) and every record it held is
    // used.  Decided in chunk order, BEFORE the chunk is run: chunks behind the end never touch a counter.
    Step end_of_input(Turn& t) {
        Job& j = t.j;
        const aqc_frame_info& info = t.info;
        const bool fin1 = j.c[0].final, fin2 = nf == 2 ? j.c[1].final : fin1;
        const bool done1 = (info.eof1 || fin1) && info.avail1 == info.n;
        const bool done2 = nf == 2 && (info.eof2 || fin2) && info.avail2 == info.n;
        const bool stop = done1 || (done2 && info.avail1 > info.n);
        std::unique_lock<std::mutex> lk(fr_mu);
        fr_cv.wait(lk, [&] { return abort.load() || framed_next == j.idx; });
        if (abort) return Step::quit;
        const bool behind_end = end_chunk != UINT64_MAX;
        bool foreign = false;
        if (!behind_end) {
            if (stop) {
                end_chunk = j.idx;
                extra_bases = (!done1 && done2 && info.avail1 > info.n) ? info.next_len1 : 0;
                j.last = true;
            } else if (info.n != K) foreign = true;      // neither K records nor an end: nothing upstream's reader could have produced from these chunks
        }
        framed_next = j.idx + 1;
        lk.unlock();
        fr_cv.notify_all();
        if (foreign) { anomaly = true; t.drop_input(); stop_all(); return Step::quit; }
        if (behind_end) return Step::skip;
        if (stop) end_input();
        return Step::go;
    }

    // post-filter QC while TOTAL_READS < qc_sample (preprocesser.py:624-627), issued in chunk order
    bool qc_turn(Turn& t) {
        const uint64_t idx = t.j.idx, g0 = t.ch.first_index;
        uint64_t n_qc = t.n;
        if (opt->qc_sample > 0) n_qc = (uint64_t)opt->qc_sample - 1 > g0 ? std::min<uint64_t>(t.n, (uint64_t)opt->qc_sample - 1 - g0) : 0;
        const bool may_qc = opt->qc_sample <= 0 || g0 < (uint64_t)opt->qc_sample - 1;
        if (!may_qc) {
            // (chunks behind the sample never wait; the turn counter is passed on by the ones before)
            std::lock_guard<std::mutex> g(qc_mu);
            if (qc_next == idx) { qc_next = idx + 1; qc_cv.notify_all(); }
            return true;
        }
        int rc = 0;
        std::unique_lock<std::mutex> lk(qc_mu);
        qc_cv.wait(lk, [&] { return abort || qc_next == idx; });
        if (!abort && n_qc > 0) {
            rc = aqc_qc_stat(t.c, t.slot, AQC_QC_R1_POST, 0, 0, n_qc, 1);
            if (!rc && nf == 2) rc = aqc_qc_stat(t.c, t.slot, AQC_QC_R2_POST, 1, 0, n_qc, 1);
            if (!rc) rc = aqc_sync(t.c, t.slot);
        }
        qc_next = idx + 1;
        lk.unlock();
        qc_cv.notify_all();
        if (rc && !dies_at_record(t, rc)) { fail(rc, "aqc_qc_stat: %s", aqc_last_error()); return false; }
        return true;
    }

    // format -> (compress) -> fetch into output set `set`, the fetch under the download gate.  A second round only when the device
    // reports, as late as the download, that upstream's run ends at a record of this chunk: the records before it are formatted
    // again on their own.
    bool format_and_fetch(Turn& t, OutChunk& oc, int set) {
        GatePass down(*this);
        bool have_set = false;
        uint64_t n_ev[2] = {0, 0};
        for (int round = 0; ; ++round) {
            const char* where = "aqc_format";
            int rc = spans_on ? aqc_format_spans(t.c, t.slot, t.n, opt->store_overlap, oc.sizes, n_ev) : aqc_format(t.c, t.slot, t.n, opt->store_overlap, oc.sizes);
            if (!rc) oc.fused = aqc_format_fused(t.c, t.slot) == 1;
            if (!rc && !have_set) {
                ns_kernels += now_ns() - t.tt;
                t.tt = now_ns();
                if (!acquire_set(t.wid, set)) return false;
                have_set = true;
                ns_wait_set += now_ns() - t.tt;
                t.tt = now_ns();
            }
            oc.gz = gz_on_device;
            if (!rc && oc.gz) { where = "aqc_compress"; rc = aqc_compress(t.c, t.slot, io->gzip_level, oc.gz_sizes); }
            if (!rc) {
                if (!down.held() && !down.enter(*down_gate[group_of_ctx[t.ci]], t.j.ticket)) return false;
                where = "fetching the output streams";
                if (!fetch_streams(t, oc, set, rc)) return false;
                if (!rc && spans_on && !fetch_spans(t, oc, set, n_ev, rc)) return false;
            }
            if (!rc) break;
            if (round == 0 && !t.fatal && dies_at_record(t, rc)) continue;
            fail(rc, "%s: %s", where, aqc_last_error());
            return false;
        }
        down.leave();
        ns_fetch += now_ns() - t.tt;
        return true;
    }
    // the six streams with one wait (aqc_fetch_streams); false: the run has failed here, else rc says how the fetch went
    bool fetch_streams(Turn& t, OutChunk& oc, int set, int& rc) {
        uint8_t* dstq[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        uint64_t capq[6] = {0, 0, 0, 0, 0, 0};
        for (int q = 0; q < 6; ++q) {
            if (!oc.sizes[q]) continue;
            HostBuf& hb = P->wbufs[t.wid].out[set][q];
            hb.ensure(oc.gz ? oc.gz_sizes[q] : oc.sizes[q]);
            if (!hb.p) { fail(AQC_ERR_HIP, "page-locked allocation failed"); return false; }
            dstq[q] = hb.p; capq[q] = hb.cap;
        }
        rc = aqc_fetch_streams(t.c, t.slot, oc.gz ? 1 : 0, dstq, capq);
        return true;
    }
    // spans mode: where the rebuilt and the bad records stood — everything between them is written from the input buffer, by the
    // file writers (the chunk keeps its input buffers) or, assembled here, as one stream.  false / rc: as fetch_streams.
    bool fetch_spans(Turn& t, OutChunk& oc, int set, const uint64_t n_ev[2], int& rc) {
        auto sp = std::make_shared<OutChunk::Spans>();
        for (int f = 0; f < nf && !rc; ++f) {
            sp->ev[f].resize((size_t)n_ev[f]);
            rc = aqc_fetch_span_events(t.c, t.slot, f, sp->ev[f].data(), n_ev[f]);
            sp->in[f] = t.j.c[f].data;
            sp->end[f] = t.n == t.info.n ? (f == 0 ? t.info.consumed1 : t.info.consumed2) : 0;
        }
        if (!rc && t.n != t.info.n) {
            // (the chunk was cut at the record upstream dies at: the last piece ends where that record begins)
            uint64_t e2[2] = {0, 0};
            rc = aqc_span_end(t.c, t.slot, t.n, e2);
            sp->end[0] = e2[0]; sp->end[1] = e2[1];
        }
        if (rc) return true;
        for (int f = 0; f < nf; ++f) {
            uint64_t total = 0;
            walk_spans(sp->ev[f].data(), 0, sp->ev[f].size(), sp->end[f], [&](uint64_t, uint64_t len) { total += len; }, [&](uint64_t len) { total += len; });
            sp->good_total[f] = total;
        }
        if (!spans_assemble) {
            oc.spans = sp;
            for (int f = 0; f < nf; ++f) oc.in_buf[f] = t.in[f].hand_on();
            return true;
        }
        // the good output of each file, put together here: the chunk's own bytes between the events, the rebuilt
        // records at them — on the pool, a task per ~1 MiB of output; then the input buffers are free again
        for (int f = 0; f < nf; ++f) {
            HostBuf& gb = P->wbufs[t.wid].good[set][f];
            gb.pageable = true;
            gb.ensure((size_t)sp->good_total[f] + 64);
            if (sp->good_total[f] && !gb.p) { fail(AQC_ERR_HIP, "allocation of a good-output buffer failed"); return false; }
            assemble_good(*sp, f, oc.sizes[3 * f] ? P->wbufs[t.wid].out[set][3 * f].p : nullptr, gb.p);
            oc.good_ptr[f] = gb.p;
            oc.good_bytes[f] = sp->good_total[f];
        }
        t.drop_input();
        return true;
    }
    // no output: the chunk still takes its turn at the download gate, then waits for its kernels
    bool sync_only(Turn& t) {
        {
            GatePass down(*this);
            if (!down.enter(*down_gate[group_of_ctx[t.ci]], t.j.ticket)) return false;
        }
        const int rc = aqc_sync(t.c, t.slot);
        if (rc && !dies_at_record(t, rc)) { fail(rc, "aqc_sync: %s", aqc_last_error()); return false; }
        return true;
    }

    // The good output of file f of a chunk formatted by aqc_format_spans -> dst (what capi.assemble_spans does in the tests, and what
    // the writev of the other spans mode hands the kernel piece by piece): the copies run on the pool, cut into tasks at events
    // (a clean chunk has few events: a long run of untouched records then makes one task's copy).
    void assemble_good(const OutChunk::Spans& sp, int f, const uint8_t* patch, uint8_t* dst) {
        const aqc_span_event* ev = sp.ev[f].data();
        const size_t n_ev = sp.ev[f].size();
        const uint8_t* in = sp.in[f];
        const uint64_t TASK = 1u << 20;
        // where each task starts: event index, output offset, patch offset
        struct Cut { size_t e; uint64_t out, poff; };
        std::vector<Cut> cuts{Cut{0, 0, 0}};
        size_t e = 0;
        uint64_t out = 0, poff = 0;
        walk_spans(ev, 0, n_ev, 0, [&](uint64_t, uint64_t len) { out += len; },
                   [&](uint64_t len) {
                       out += len; poff += len; ++e;
                       if (out - cuts.back().out >= TASK) cuts.push_back(Cut{e, out, poff});
                   });
        P->pool->parallel_for(cuts.size(), [&](size_t t) {
            const bool last = t + 1 == cuts.size();
            uint64_t o = cuts[t].out, po = cuts[t].poff;
            walk_spans(ev, cuts[t].e, last ? n_ev : cuts[t + 1].e, last ? sp.end[f] : 0,
                       [&](uint64_t at, uint64_t len) { memcpy(dst + o, in + at, (size_t)len); o += len; },
                       [&](uint64_t len) { if (len) { memcpy(dst + o, patch + po, (size_t)len); o += len; po += len; } });
        });
    }

    // An exception INSIDE upstream's loop (KeyError / IndexError of the overlap walk, int() of a name field) ends its run at that
    // record with everything before it written.  The device reports the earliest such record of the chunk (aqc_error_record): the
    // chunk is cut there and becomes the run's last one — the writer commits it in its turn, then the pipe stops and aqc_pipe_run
    // returns the error.  (Chunks are committed in order: a death in a later chunk never overtakes an earlier chunk's records.)
    bool dies_at_record(Turn& t, int rc) {
        if (rc != AQC_ERR_INDEX && rc != AQC_ERR_ALPHABET && rc != AQC_ERR_ARG) return false;
        uint64_t rec = UINT64_MAX;
        if (aqc_error_record(t.c, t.slot, &rec) || rec == UINT64_MAX || rec >= t.n) return false;
        {
            std::lock_guard<std::mutex> g(err_mu);
            if (fatal_chunk == UINT64_MAX || t.j.idx < fatal_chunk) {
                fatal_chunk = t.j.idx;
                fatal_err = aqc_last_error();
                fatal_code = rc;
            }
        }
        t.n = rec;
        t.fatal = true;
        return true;
    }

    // ---- commit in chunk order, one writer per file -----------------------------------------------------------------------------------
    // What output file q receives from a chunk, and how many bytes of text that is (what bytes_out counts; a device-made .gz
    // stream is gz_sizes[q] bytes in the file).  Read by the commit thread (whom to queue it for) and by the file writer (what to write).
    enum class Feed { nothing, assembled, spans, stream, device_gz };
    struct Share { Feed kind; uint64_t bytes; };
    Share share_of(const OutChunk& oc, int q) const {
        const int f = q / 3;
        uint64_t bytes = oc.sizes[q];
        Feed kind = !io->gzip_out ? Feed::stream : oc.gz ? Feed::device_gz : Feed::stream;
        if (q % 3 == 0 && oc.good_ptr[f]) { kind = Feed::assembled; bytes = oc.good_bytes[f]; }       // the slot worker has put the chunk's good output together
        else if (q % 3 == 0 && oc.spans) { kind = Feed::spans; bytes = oc.spans->good_total[f]; }    // the chunk's own bytes between the events, the rebuilt records at them
        return Share{bytes ? kind : Feed::nothing, bytes};
    }

    void file_writer(int q) {
        bind_io_thread("file writer");
        std::shared_ptr<Commit> cm;
        while (fileq[q]->pop(cm)) {
            const OutChunk& oc = cm->oc;
            const uint64_t tw = now_ns();
            const Share sh = abort ? Share{Feed::nothing, 0} : share_of(oc, q);
            const uint8_t* p = oc.set >= 0 ? P->wbufs[oc.worker].out[oc.set][q].p : nullptr;      // stream q as the device made it
            bool ok = true;
            switch (sh.kind) {
            case Feed::nothing: break;
            case Feed::assembled: ok = out[q].append(oc.good_ptr[q / 3], (size_t)sh.bytes); break;
            case Feed::spans: {
                // the good file of input q / 3: the rebuilt records are stream q
                const OutChunk::Spans& sp = *oc.spans;
                const int f = q / 3;
                std::vector<struct iovec> iov;
                iov.reserve(2 * sp.ev[f].size() + 1);
                uint64_t poff = 0;
                walk_spans(sp.ev[f].data(), 0, sp.ev[f].size(), sp.end[f],
                           [&](uint64_t at, uint64_t len) { iov.push_back({(void*)(sp.in[f] + at), (size_t)len}); },
                           [&](uint64_t len) { if (len) { iov.push_back({(void*)(p + poff), (size_t)len}); poff += len; } });
                ok = out[q].appendv(iov);
                break;
            }
            case Feed::device_gz: ok = out[q].append(p, (size_t)oc.gz_sizes[q]); break;
            case Feed::stream: ok = io->gzip_out ? append_bgzf(q, p, (size_t)sh.bytes) : out[q].append(p, (size_t)sh.bytes); break;
            }
            if (!ok) fail(AQC_ERR_ARG, "write error on output %d (disk full?)", q);
            ns_write += now_ns() - tw;
            if (cm->remaining.fetch_sub(1) == 1) release_set(oc);
            writes_done.fetch_add(1);
        }
    }
    // text -> BGZF members deflated on the pool -> file q
    bool append_bgzf(int q, const uint8_t* p, size_t n) {
        const size_t blk = 0xff00;                    // BGZF: at most 64 KiB per member, headers included (stored: text + 31 bytes)
        const size_t nb = (n + blk - 1) / blk;
        std::vector<std::vector<uint8_t>> z(nb);
        P->pool->parallel_for(nb, [&](size_t i) {
            const size_t o = i * blk;
            bgzf_block(p + o, std::min<size_t>(blk, n - o), io->gzip_level, z[i]);
        });
        size_t total = 0;
        for (auto& b : z) total += b.size();
        std::vector<uint8_t> cat(total);
        size_t o = 0;
        for (auto& b : z) { memcpy(cat.data() + o, b.data(), b.size()); o += b.size(); }
        return out[q].append(cat.data(), total);
    }

    void writer() {
        bind_io_thread("commit");
        std::map<uint64_t, OutChunk> pending;
        uint64_t next = 0;
        OutChunk oc;
        bool done = false;
        while (!done && outq.pop(oc)) {
            pending[oc.idx] = oc;
            while (!pending.empty() && pending.begin()->first == next) {
                OutChunk cur = pending.begin()->second;
                pending.erase(pending.begin());
                auto cm = std::make_shared<Commit>();
                cm->oc = cur;
                int live = 0;
                bool to_file[6];
                for (int q = 0; q < 6; ++q) {
                    const Share sh = share_of(cur, q);
                    res->bytes_out[q] += sh.bytes;
                    to_file[q] = sh.kind != Feed::nothing && out[q].fd >= 0;
                    if (cur.set >= 0 && to_file[q]) ++live;
                }
                if (live == 0 || abort) release_set(cur);
                else {
                    cm->remaining = live;
                    for (int q = 0; q < 6; ++q)
                        if (to_file[q]) { writes_queued.fetch_add(1); fileq[q]->push(cm); }
                }
                res->chunks += 1;
                res->fused_chunks += cur.fused ? 1 : 0;
                ++next;
                if (cur.fatal) fatal_commit = cm;
                if (cur.last) { done = true; break; }
            }
        }
        outq.close();
        for (int q = 0; q < 6; ++q) fileq[q]->close();
        if (fatal_commit) {
            // upstream died inside this chunk: everything up to the record is on its way to the files; once it is there the
            // rest of the pipe (readers, workers with later chunks) is stopped and the run reports the error
            while (!abort && (fatal_commit->remaining.load() > 0 || writes_done.load() < writes_queued.load())) std::this_thread::sleep_for(std::chrono::microseconds(200));
            {
                std::lock_guard<std::mutex> g(err_mu);
                if (err.empty()) { err = fatal_err; err_code = fatal_code; }
            }
            stop_all();
        }
    }

    // ---- the run, from the caller's thread ------------------------------------------------------------------------------------------
    // 0, or AQC_ERR_ARG with the file named in g_pipe_err
    int open_outputs() {
        if (opt->no_output) return 0;
        for (int q = 0; q < 6; ++q) {
            const char* path = io->out_path[q / 3][q % 3];
            if (!path) continue;
            if (!out[q].open_(path)) {
                snprintf(g_pipe_err, sizeof(g_pipe_err), "cannot open %s for writing", path);
                for (int k = 0; k < q; ++k) out[k].close_();
                return AQC_ERR_ARG;
            }
        }
        return 0;
    }
    template <class Body>
    void timed(int kind, Body&& body) {
        body();
        cpu_us[kind] += (long)(thread_cpu_s() * 1e6);
    }
    void run_threads(double t0) {
        cpu_proc0 = process_cpu_s();
        cpu_pool0 = dbg ? P->pool->cpu_seconds() : 0.0;
        std::vector<std::thread> fw;
        for (int q = 0; q < 6; ++q)
            if (out[q].fd >= 0) fw.emplace_back([this, q] { timed(0, [&] { file_writer(q); }); });
        std::vector<std::thread> th;
        for (int f = 0; f < nf; ++f) th.emplace_back([this, f] { timed(1, [&] { reader(f); }); });
        th.emplace_back([this] { timed(2, [&] { dispatcher(); }); });
        for (int ci = 0; ci < P->n_ctx; ++ci)
            for (int s = 0; s < P->slots; ++s) th.emplace_back([this, ci, s] { timed(3, [&] { worker(ci, s); }); });
        std::thread wr([this] { timed(4, [&] { writer(); }); });
        for (auto& t : th) t.join();
        if (dbg) fprintf(stderr, "pipe: readers / workers done at %.4f s\n", now_s() - t0);
        // all producers are done: if the last chunk never arrived (abort / anomaly) the writer must not wait for it
        outq.close();
        wr.join();
        for (auto& t : fw) t.join();
        if (dbg) fprintf(stderr, "pipe: writers done at %.4f s\n", now_s() - t0);
    }
    void close_outputs() {
        for (int q = 0; q < 6; ++q) {
            if (out[q].fd < 0) continue;
            if (io->gzip_out && !abort) {
                // an empty BGZF member terminates the file (and makes an output with no records a valid .gz)
                std::vector<uint8_t> e;
                bgzf_block((const uint8_t*)"", 0, io->gzip_level, e);
                (void)out[q].append(e.data(), e.size());
            }
            out[q].close_();
        }
    }
    void debug_report(double t0) {
        fprintf(stderr, "pipe: files closed at %.4f s\n", now_s() - t0);
        const double proc = process_cpu_s() - cpu_proc0, pool = P->pool->cpu_seconds() - cpu_pool0;
        double named = 0;
        for (auto& c : cpu_us) named += 1e-6 * (double)c.load();
        fprintf(stderr, "pipe: CPU seconds — process %.3f = pool %.3f + readers %.3f + dispatcher %.3f + slot workers %.3f + commit %.3f + file writers %.3f + other threads (GPU runtime, caller) %.3f\n",
                proc, pool, 1e-6 * cpu_us[1], 1e-6 * cpu_us[2], 1e-6 * cpu_us[3], 1e-6 * cpu_us[4], 1e-6 * cpu_us[0], proc - pool - named);
        uint64_t ds[8];
        aqcgz::device_offload_stats(ds);
        if (ds[5]) fprintf(stderr, "pipe: device gunzip so far (process-wide) — %llu groups, %llu sections given / %llu found; ms in scan %.1f, decode %.1f, chain + gather %.1f, H2D %.1f, D2H %.1f\n",
                           (unsigned long long)ds[5], (unsigned long long)ds[6], (unsigned long long)ds[7], ds[0] / 1e3, ds[1] / 1e3, ds[2] / 1e3, ds[3] / 1e3, ds[4] / 1e3);
        uint64_t rs[4];
        aqcgz::device_resolve_stats(rs);
        if (rs[0]) fprintf(stderr, "pipe: markers + CRC-32 resolved on the device so far (process-wide) — %llu runs of %llu sections, %.1f MB of text, %.1f ms inside resolve()\n",
                           (unsigned long long)rs[0], (unsigned long long)rs[1], 1e-6 * (double)rs[3], rs[2] / 1e3);
#ifdef AQC_GZ_PROFILE
        fprintf(stderr, "pipe: gunzip thread-CPU ms — find %ld, decode (find included) %ld, translate %ld, crc %ld, consumer waiting %ld, accept %ld\n", aqcgz::gz_prof[0].exchange(0) / 1000,
                aqcgz::gz_prof[1].exchange(0) / 1000, aqcgz::gz_prof[2].exchange(0) / 1000, aqcgz::gz_prof[3].exchange(0) / 1000, aqcgz::gz_prof[4].exchange(0) / 1000, aqcgz::gz_prof[5].exchange(0) / 1000);
#endif
    }
    // the run's error, if any, into g_pipe_err: its code (`dflt` where the failure named none), or 0
    int report_error(int dflt) {
        if (err.empty()) return 0;
        std::lock_guard<std::mutex> g(g_pipe_err_mu);
        snprintf(g_pipe_err, sizeof(g_pipe_err), "%s", err.c_str());
        return err_code ? err_code : dflt;
    }
};

}  // namespace

// CPUs' worth of run time the cgroup grants (v2: cpu.max, v1: cpu.cfs_quota_us / cpu.cfs_period_us); 0 = no limit / unknown
static double cgroup_cpu_quota() {
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64]; long long per = 0;
        const int k = fscanf(f, "%63s %lld", q, &per);
        fclose(f);
        if (k == 2 && strcmp(q, "max") != 0 && per > 0) return (double)atoll(q) / (double)per;
        return 0;
    }
    long long q = -1, per = 0;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(f, "%lld", &q) != 1) q = -1; fclose(f); }
    if (FILE* f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(f, "%lld", &per) != 1) per = 0; fclose(f); }
    return (q > 0 && per > 0) ? (double)q / (double)per : 0;
}

extern "C" {

const char* aqc_pipe_last_error(void) { return g_pipe_err; }

int aqc_pipe_create(aqc_ctx** ctxs, int32_t n_ctx, int32_t slots_per_ctx, int32_t io_threads, aqc_pipe** out) {
    if (!ctxs || n_ctx < 1 || !out || slots_per_ctx < 1 || slots_per_ctx > 16) return AQC_ERR_ARG;
    aqc_pipe* p = new aqc_pipe();
    p->n_ctx = n_ctx;
    p->ctx.assign(ctxs, ctxs + n_ctx);
    p->slots = slots_per_ctx;
    unsigned hc = std::thread::hardware_concurrency();
    // default pool: three eighths of the machine's hardware threads (96 on the 2 x 64-core MI355X hosts), shared fairly when
    // several ranks run on one node (torchrun exports LOCAL_WORLD_SIZE); gzip work (speculative inflate sections, deflate of
    // independent members) is what scales with it
    unsigned share = 1;
    if (const char* lw = getenv("LOCAL_WORLD_SIZE")) share = (unsigned)std::max(1, atoi(lw));
    unsigned dflt = std::min(96u, std::max(4u, hc * 3 / 8 / share));
    // ... but not beyond what the container may actually use: under a cgroup CPU quota (the MI355X boxes: 256 hardware threads
    // visible, cpu.max = 16 CPUs) more runnable threads get the whole group throttled in bursts and run with cold caches.
    // Measured on such a box (tools/gpu_pool_sweep.sh, 10 M reads, gzip -1 single-member input -> .gz): pool of 16 / 24 / 32 / 48 / 64 /
    // 96 threads = 0.45 / 0.48 / 0.46 / 0.55 / 0.62 / 0.69 s; plain files 16 / 32 / 64 = 0.25 / 0.27 / 0.29 s.
    const double quota = cgroup_cpu_quota();
    if (quota > 0) dflt = std::min(dflt, std::max(4u, (unsigned)(quota * 1.25 / share + 0.5)));
    if (io_threads <= 0)
        if (const char* e = getenv("AQC_IO_THREADS")) io_threads = std::min(256, atoi(e));
    p->io_threads = io_threads > 0 ? io_threads : (int)dflt;
    p->pool.reset(new Pool(p->io_threads));
    // input buffers: one per slot + two being filled — and, when the good records are written straight from them (spans mode), the
    // two chunks per slot worker that may wait for their turn at the files (buffers are page-locked when first used, not before)
    const int ring = n_ctx * slots_per_ctx * 3 + 2;
    for (int f = 0; f < 2; ++f) p->in_buf[f].resize(ring);
    p->wbufs.resize((size_t)n_ctx * slots_per_ctx);
    *out = p;
    return 0;
}

void aqc_pipe_destroy(aqc_pipe* p) {
    if (!p) return;
    // the device decoders stay for the next pipe
    for (auto& d : p->dec) { d.gz.give_back(g_gz_keep); d.bz2.give_back(g_bz2_keep); }
    delete p;       // (its buffers free themselves, here: HostBuf)
}

int aqc_pipe_run(aqc_pipe* P, const aqc_pipe_io* io, const aqc_pipe_opts* opt, aqc_pipe_result* res) {
    if (!P || !io || !opt || !res) return AQC_ERR_ARG;
    memset(res, 0, sizeof(*res));
    if (!io->in_path[0] && !io->in_mem[0]) return AQC_ERR_ARG;
    const double t0 = now_s();
    Run R(P, io, opt, res);
    if (const int rc = R.open_outputs()) return rc;
    if (R.dbg) fprintf(stderr, "pipe: outputs open at %.4f s\n", now_s() - t0);
    R.run_threads(t0);
    R.close_outputs();
    if (R.dbg) R.debug_report(t0);
    res->records = R.records.load();
    res->t_read = 1e-9 * (double)R.ns_read.load(); res->t_count = 1e-9 * (double)R.ns_count.load();
    res->t_frame = 1e-9 * (double)R.ns_frame.load(); res->t_kernels = 1e-9 * (double)R.ns_kernels.load();
    res->t_fetch = 1e-9 * (double)R.ns_fetch.load(); res->t_write = 1e-9 * (double)R.ns_write.load();
    res->t_wait_set = 1e-9 * (double)R.ns_wait_set.load(); res->t_wait_ring = 1e-9 * (double)R.ns_wait_ring.load();
    res->anomaly = R.anomaly ? 1 : 0;
    res->extra_bases = R.extra_bases;
    res->seconds = now_s() - t0;
    return R.report_error(AQC_ERR_HIP);
}

// ---- byte sources on their own: what fastq.Reader's file object is upstream (fastq.py:23-28), with the pipe's readers behind
//      it (parallel pread; BGZF members inflated in parallel; other gzip data through one zlib stream)
struct aqc_source {
    std::unique_ptr<Pool> pool;
    std::unique_ptr<Source> src;
};

aqc_source* aqc_source_open2(const char* path, int32_t gzip, int32_t io_threads, uint64_t gz_section_bytes) {
    if (!path) return nullptr;
    aqc_source* s = new aqc_source();
    unsigned hc = std::thread::hardware_concurrency();
    s->pool.reset(new Pool(io_threads > 0 ? io_threads : (int)std::min(16u, std::max(2u, hc / 4))));
    if (gzip == 2) s->src.reset(new Bz2Source(path, s->pool.get()));
    else if (gzip) s->src.reset(new GzSource(path, s->pool.get(), (size_t)gz_section_bytes));
    else s->src.reset(new FileSource(path, s->pool.get()));
    if (s->src->failed()) { delete s; return nullptr; }
    return s;
}

aqc_source* aqc_source_open(const char* path, int32_t gzip, int32_t io_threads) { return aqc_source_open2(path, gzip, io_threads, 0); }

const char* aqc_source_error(aqc_source* s) { return s && s->src->failed() ? s->src->why() : ""; }

int aqc_source_gz_stats(aqc_source* s, uint64_t out[4]) {
    if (!s || !out) return AQC_ERR_ARG;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (GzSource* g = dynamic_cast<GzSource*>(s->src.get()))
        if (g->pg) { out[0] = g->pg->sections_accepted; out[1] = g->pg->sections_discarded; out[2] = g->pg->bridged_bytes; out[3] = g->pg->total_out; }
    return 0;
}

int aqc_gz_input_stats(uint64_t out[4]) {
    if (!out) return AQC_ERR_ARG;
    for (int i = 0; i < 4; ++i) out[i] = g_gz_in_stats[i].load();
    return 0;
}

int aqc_bz2_input_stats(uint64_t out[4]) {
    if (!out) return AQC_ERR_ARG;
    for (int i = 0; i < 4; ++i) out[i] = g_bz2_in_stats[i].load();
    return 0;
}

int aqc_gz_deflate_block(const uint8_t* src, uint64_t n, int32_t level, uint8_t* dst, uint64_t cap, uint64_t* out_n) {
    if ((!src && n) || !dst || !out_n || cap < aqcgz::deflate_bound((size_t)n)) return AQC_ERR_ARG;
    *out_n = aqcgz::deflate_block(src, (size_t)n, level, dst);
    return 0;
}

int64_t aqc_gz_inflate_raw(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap) {
    if (!src || (!dst && cap)) return -1;
    return aqcgz::inflate_raw(src, (size_t)n, dst, (size_t)cap);
}

uint32_t aqc_gz_crc32(uint32_t crc, const uint8_t* p, uint64_t n) { return aqcgz::crc32_fast(crc, p, (size_t)n); }

int64_t aqc_source_read(aqc_source* s, uint8_t* dst, uint64_t want) {
    if (!s || (!dst && want)) return -1;
    const size_t got = want ? s->src->read(dst, (size_t)want) : 0;
    if (s->src->failed()) return -1;
    return (int64_t)got;
}

void aqc_source_close(aqc_source* s) { delete s; }

// ---- host-only helpers (no GPU involved): used by the CPU tests of the pipe's reader / writer halves ---------------------
uint64_t aqc_host_count_newlines(const uint8_t* p, uint64_t n) { return p ? count_nl(p, (size_t)n) : 0; }

int aqc_bgzf_compress(const uint8_t* src, uint64_t n, int32_t level, uint8_t* dst, uint64_t cap, uint64_t* out_n) {
    if ((!src && n) || !dst || !out_n) return AQC_ERR_ARG;
    const size_t blk = 0xff00;
    uint64_t o = 0;
    std::vector<uint8_t> z;
    for (uint64_t i = 0; i < n || (n == 0 && i == 0); i += blk) {
        bgzf_block(src + i, (size_t)std::min<uint64_t>(blk, n - i), level, z);
        if (o + z.size() > cap) return AQC_ERR_ARG;
        memcpy(dst + o, z.data(), z.size());
        o += z.size();
        if (n == 0) break;
    }
    *out_n = o;
    return 0;
}

// one reader of the pipe on its own: a pipe without contexts whose two ring buffers are plain memory, a run without output
int aqc_pipe_split(const aqc_pipe_io* io, int32_t file_index, uint64_t chunk_records, int32_t io_threads, uint64_t* bytes,
                   uint64_t* lines, uint64_t cap, uint64_t* n_chunks, uint32_t* crc) {
    if (!io || file_index < 0 || file_index > 1 || !n_chunks || !crc) return AQC_ERR_ARG;
    aqc_pipe P;
    P.n_ctx = 0;
    P.io_threads = io_threads > 0 ? io_threads : 4;
    P.pool.reset(new Pool(P.io_threads));
    for (int f = 0; f < 2; ++f) {
        P.in_buf[f].resize(2);
        for (auto& b : P.in_buf[f]) b.pageable = true;
    }
    aqc_pipe_opts opt{};
    opt.chunk_records = chunk_records;
    opt.no_output = 1;
    aqc_pipe_result res{};
    const int f = file_index;
    Run R(&P, io, &opt, &res, f);
    std::thread rd([&R, f] { R.reader(f); });
    uint64_t k = 0;
    uint32_t c = (uint32_t)crc32(0L, Z_NULL, 0);
    InChunk ch;
    while (R.inq[f]->pop(ch)) {
        if (k < cap) { if (bytes) bytes[k] = ch.bytes; if (lines) lines[k] = ch.lines; }
        for (uint64_t o = 0; o < ch.bytes; o += (1u << 30)) c = (uint32_t)crc32(c, ch.data + o, (uInt)std::min<uint64_t>(1u << 30, ch.bytes - o));
        ++k;
        R.release_ring(f, ch.buf);
    }
    rd.join();
    *n_chunks = k;
    *crc = c;
    return R.report_error(AQC_ERR_ARG);
}

}  // extern "C"
