// aqc_ctx.hpp — what the C-API translation units of libafterqc_hip.so (aqc_capi.hip and aqc_capi_run / _qc / _text.hip) share on
// the host side: the context and its slots, the constants that size their buffers, and the helpers every entry point goes through
// (find the slot, wait for it, read what its kernels reported, copy a result out).  Each unit owns the entry points of one stage
// and is the only one to include that stage's kernel-defining device headers; this header includes none of them, only the
// descriptors (aqc_batch.hpp).  Internal: nothing here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "aqc_dev.hpp"
#include "aqc_batch.hpp"
#include "aqc_qcut.hpp"
#include "aqc_adapter.hpp"
#include "aqc_polytail.hpp"
#include "aqc_adpcensus.hpp"

namespace aqc {

// The passes in front of the verdict kernel that leave a view per mate and record in Slot::cut (aqc_viewpass.hpp), in launch order
enum ViewPassId { VP_CUT = 0, VP_ADAPTER = 1, VP_POLY = 2, VP_N = 3 };
// ... what a slot keeps of each: the event pair around the pass of the last aqc_run (aqc_cut_ms / aqc_adapter_ms / aqc_poly_ms), if it launched one
struct ViewPass { hipEvent_t ev[2] = {nullptr, nullptr}; bool ran = false; };
// ... and what the context keeps: [4] reads of R1 the pass made shorter, bases it took from them, the same for R2.  On the device
// from the first time the pass is switched on: a context that never sets it allocates what it always did.
struct __attribute__((visibility("hidden"))) PassCounts {
    unsigned long long* p = nullptr;
    hipError_t ensure(int device) {
        if (p) return hipSuccess;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc((void**)&p, sizeof(unsigned long long) * 4);
        return e == hipSuccess ? zero() : e;
    }
    hipError_t zero() { return p ? hipMemset(p, 0, sizeof(unsigned long long) * 4) : hipSuccess; }
    hipError_t get(int64_t out[4]) const {
        for (int k = 0; k < 4; ++k) out[k] = 0;
        return p ? hipMemcpy(out, p, sizeof(int64_t) * 4, hipMemcpyDeviceToHost) : hipSuccess;
    }
    void free() { if (p) (void)hipFree(p); p = nullptr; }
};

// What a slot holds once per input file (mate 0 = read 1, mate 1 = read 2), grouped like the slot itself by the unit that fills it.
struct __attribute__((visibility("hidden"))) Mate {
    // ---- upload and verdicts (aqc_capi_run.hip; aqc_frame fills the same arena and tables from text) ----
    DevBuf seq, qual, off, qoff, len;    // arena (framed text sits TEXT_FRONT bytes in), quality arena, byte offsets, quality offsets, lengths
    DevBuf qlen, qview;                  // quality-line lengths of an uploaded batch (aqc_batch::qlen*), final quality views of LEN_IRR records
    DevBuf fz_rec;                       // AQC_FUSED=1: position words per record (see Slot::fz_state)
    // ---- text in, text out (aqc_capi_text.hip) ----
    DevBuf line_end, name_off, name_len, plus_off, plus_len, qual_len;   // the line table and the name / strand-line / quality-length descriptors
    uint8_t last_byte = '\n';
    uint64_t consumed = 0;               // bytes of the file's chunk that the framed records take
    DevBuf f_events;                     // aqc_format_spans: the file's events ...
    uint64_t n_events = 0;               // ... and how many
};

// One mate of a batch view, as pointers; set_mate writes it into a DevBatch.  The single-end rules are here and nowhere else:
// mate 0 also stands in for mate 1's quality words (qlen2 = qlen1, qview2 = qview1) until a mate 1 is set, and a single-end
// aqc_frame hands frame_finish_kernel line table 0 twice (the kernel takes two tables whatever the chunk holds).
struct MateView { const uint8_t *seq, *qual; const uint32_t *off, *qoff, *len, *qlen; uint32_t* qview; };
static inline void set_mate(DevBatch& v, int k, const MateView& m) {
    if (k == 0) { v.seq1 = m.seq; v.qual1 = m.qual; v.off1 = m.off; v.qoff1 = m.qoff; v.len1 = m.len; v.qlen1 = v.qlen2 = m.qlen; v.qview1 = v.qview2 = m.qview; }
    else { v.seq2 = m.seq; v.qual2 = m.qual; v.off2 = m.off; v.qoff2 = m.qoff; v.len2 = m.len; v.qlen2 = m.qlen; v.qview2 = m.qview; }
}

// One slot of a context.  A slot's fields are grouped by the unit whose entry points fill them; a later stage reads what an
// earlier one left (aqc_format the verdicts and the framing, aqc_compress the formatted streams).
struct __attribute__((visibility("hidden"))) Slot {
    // ---- every unit (aqc_capi.hip): the stream, the error words, the order against the QC stream, launch timing ----
    hipStream_t stream = nullptr;
    int* status = nullptr;           // first device-side error raised by this slot's kernels (one word per slot: the slots
                                     // of a context may be driven from different host threads); 16 bytes: the word, and at
                                     // byte 8 DevStats::err_key (the earliest record at which upstream's run would have died)
    uint64_t err_record = UINT64_MAX; // ... as the last check_status read it (aqc_error_record)
    hipEvent_t ev_main = nullptr, ev_qc = nullptr;     // ordering between the slot's stream and the context's QC stream
    // QC kernels of this slot may still run on the QC stream: `gen` counts the aqc_qc_stat calls (bumped AFTER ev_qc is recorded),
    // `synced` how many of them somebody has waited for.  Two threads may look at one slot at a time — the thread that drives
    // it and another thread's aqc_get_qc / aqc_get_kmers, which synchronise every slot (the round-3 advisory: a plain flag that
    // either of them cleared could swallow the other's newer launch).  A waiter only ever marks what it has seen.
    struct QcGen {
        std::atomic<uint64_t> gen{0}, synced{0};
        bool pending() const { return synced.load(std::memory_order_acquire) < gen.load(std::memory_order_acquire); }
    } qc;
    hipEvent_t ev[AQC_N_KERNELS][2] = {};
    bool timed[AQC_N_KERNELS] = {};
    // timing region (aqc_timing_reset / aqc_timing_mean): one event pair per launch
    std::vector<hipEvent_t> ring[AQC_N_KERNELS][2];
    int ring_used[AQC_N_KERNELS] = {};
    bool collecting = false;

    // ---- upload and verdicts (aqc_capi_run.hip; aqc_frame fills the same arenas and view from text) ----
    bool has_irregular = false;      // some record of the slot has a quality line that is not as long as its sequence line
    Mate m[2];                       // everything that exists once per input file
    DevBuf aux[5], results;
    DevBuf deferred, n_deferred;     // records the lane-per-read kernel hands to the general kernel
    DevBuf off_stage;                // the caller's 64-bit offsets on their way to the 32-bit device form
    uint32_t max_len = 0;
    uint32_t raw_max_len = 0;      // longest read of the slot (both mates), 0 = unknown
    DevBatch view{};
    uint64_t n = 0;
    bool paired = false, ran = false, used_fast = false;
    int verdict_words = 0;         // words per read of the lane-per-pair instance the last aqc_run launched, 0: the general kernel
    DevBuf cut;                    // the views (aqc_viewpass.hpp: one per mate and record), filled by aqc_run's view passes in front of the verdict kernel
    ViewPass pass[VP_N];
    // AQC_FUSED=1: the verdict kernel placed the slot's records in their streams and copied the whole good ones (aqc_fast.hpp, FUSE)
    DevBuf fz_state, fz_misc;                 // look-back words per batch (Mate::fz_rec: position words per record); ticket | abort | totals[4]
    bool fused = false;                       // ... for the records the slot holds now (aqc_format checks fz_misc's abort word)

    // ---- text in, text out, the census (aqc_capi_text.hip) ----
    // text in / text out (aqc_frame, aqc_format): the per-file tables are in Mate
    DevBuf t_tile;                 // the index pass's tile words, both files
    DevBuf t_scratch;              // FrameMeta[2] + scan totals (the layout: aqc_capi_text.hip)
    aqc_text_chunk last_chunk{};   // what the slot's arenas hold (aqc_reframe)
    bool framed = false, formatted = false;
    DevBuf f_pos, f_tile, f_plan, f_patch, f_over, f_out[6];
    bool formatted_fused = false;             // the last aqc_format took that placement (aqc_format_fused)
    uint64_t f_bytes[6] = {0, 0, 0, 0, 0, 0};
    // aqc_poly_census: the hits of the last census of the slot's records, and their counter
    DevBuf census_hits, census_n;
    uint64_t n_census = 0;
    hipEvent_t census_ev[2] = {nullptr, nullptr};   // around the census kernels of the last aqc_poly_census (aqc_census_ms)

    // ---- the adapter census of pass 1 (aqc_capi_qc.hip) ----
    hipEvent_t adp_census_ev[2] = {nullptr, nullptr};   // around the kernel of the slot's last aqc_adapter_census (aqc_adapter_census_ms) ...
    bool adp_census_ran = false;                        // ... if there was one

    // ---- .gz out (aqc_capi_run.hip: it is compiled beside the verdict kernels, see there) ----
    // gzip members built on the device (aqc_compress)
    DevBuf g_stage, g_sizes, g_offsets, g_total, g_hist, g_code, g_packed[6];
    uint64_t g_bytes[6] = {0, 0, 0, 0, 0, 0};
    bool compressed = false;
};

constexpr int RING_CAP = 256;

constexpr uint64_t KMER_CAP = 1ull << 21;
constexpr uint64_t DENSE_CAP = (uint64_t)N_XCD * DENSE_ENTRIES;   // 4^8 pure A/C/G/T k-mers, one copy per XCD

struct __attribute__((visibility("hidden"))) QcDev {
    unsigned long long* acc = nullptr;   // [QC_ROWS * QC_COLS]
    KmerTable kt{};
    // k-mer time keys: (epoch << 34 | global record index) * 1024 + position.  The epoch is bumped when a call
    // goes back in the file (statFile's "stat the skipped reads afterwards", qualitycontrol.py:353-355), so the
    // keys order insertions exactly like the reference's sequential dict and merge across GPUs with min().
    unsigned long long last_end = 0, epoch = 0;
};

// The adapter census of one pre-filter file (AQC_QC_R1_PRE / AQC_QC_R2_PRE): the probes aqc_set_adapter_probes gave (n 0: none) and
// the counts on the device, [0] reads looked at, [1 + i] reads that hold probe i.  Allocated when probes are first set: a context
// that never asks for the census allocates what it always did.
struct __attribute__((visibility("hidden"))) AdpCensus {
    CensusProbes probes{};
    unsigned long long* acc = nullptr;
    hipError_t ensure(int device) {
        if (acc) return hipSuccess;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc((void**)&acc, sizeof(unsigned long long) * CEN_COUNTS);
        return e;
    }
    hipError_t zero() { return acc ? hipMemset(acc, 0, sizeof(unsigned long long) * CEN_COUNTS) : hipSuccess; }
    void free() { if (acc) (void)hipFree(acc); acc = nullptr; }
};

}  // namespace aqc

struct __attribute__((visibility("hidden"))) aqc_ctx {
    bool force_generic = false;
    bool fuse_opt = false;        // AQC_FUSED=1: 2 x <=160 pairs framed on the device take the verdict kernel that also places and copies
    bool qc_inline = false;       // AQC_QC_STREAM=0: statRead kernels on the slot's stream instead of the context's QC stream
    int device = 0;
    int n_slots = 0;
    std::vector<aqc::Slot> slots;
    aqc_config cfg{};
    bool has_cfg = false;
    aqc::QcutOpts cut{};               // aqc_set_quality_cut: the quality cut (all modes 0: off, no kernel of it is launched)
    aqc::AdapterOpts adapter{};        // aqc_set_adapter_trim: the adapters to trim (both lengths 0: off, no kernel of it is launched)
    aqc::PolyOpts poly{};              // aqc_set_poly_trim: the letters whose tails are cut (every length 0: off, no kernel of it is launched)
    aqc::PassCounts pass_stats[aqc::VP_N];
    aqc::AdpCensus adp_census[2];      // aqc_set_adapter_probes: the census of read 1's / read 2's pre-filter sample (no probes: no kernel of it is launched)
    aqc::DevBuf circ[5];
    aqc::DevBuf kmer_partial;          // per-round u16 count slices of kmer_count_kernel
    aqc::DevBuf gz_crc;                // GzCrcTables (aqc_compress)
    hipStream_t qc_stream = nullptr;   // statRead kernels (latency-bound, a few thousand waves) run beside the slots' bandwidth-bound kernels
    std::mutex qc_mu;             // aqc_qc_stat calls of different slots queue up here: they share kmer_partial and the QC stream
    aqc::DevCircles circles{};
    unsigned long long *counters = nullptr, *ovl_hist = nullptr, *dist_hist = nullptr;
    aqc::QcDev qc[4];
    int n_cu = 256;
    char name[256] = "";
};

namespace aqc {

struct StatusWords { int status; int pad_; unsigned long long err_key; };
static const StatusWords STATUS_CLEAR{0, 0, ~0ull};
static unsigned long long* err_key_of(const Slot& sl) { return reinterpret_cast<unsigned long long*>(sl.status + 2); }

// (ARENA_SLACK readable bytes behind every arena: the lane-per-read kernel always loads whole 16-byte chunks, up to
// 320 bytes — 16 x the widest tier's 20 words — from the start of a read whatever its length)
constexpr size_t ARENA_SLACK = 1024;
constexpr size_t TEXT_FRONT = 64;

// ---- the helpers: defined once, in aqc_capi.hip (but for the two that belong to the statRead unit) ----
#define AQC_INTERNAL __attribute__((visibility("hidden")))
AQC_INTERNAL hipEvent_t launch_event(Slot& s, int k, int which);
AQC_INTERNAL hipError_t slot_sync(Slot& s);
AQC_INTERNAL const char* status_text(int st, bool at_record);
AQC_INTERNAL int check_status(Slot& sl);
AQC_INTERNAL int get_slot(aqc_ctx* c, int slot, Slot** out);
AQC_INTERNAL int fetch_out(Slot& s, const void* src, uint64_t bytes, void* dst, uint64_t cap, const char* who);
AQC_INTERNAL int sync_all(aqc_ctx* c);
// lanes per read of a pass in the frame of aqc_viewpass.hpp, by the slot's longest line: a quality line of its own length (or a
// length nobody has looked at) may be anything up to AQC_MAX_READ_LEN
static inline int view_pass_lanes(const Slot& s) {
    const uint32_t longest = (s.has_irregular || s.raw_max_len == 0) ? (uint32_t)AQC_MAX_READ_LEN : s.raw_max_len;
    return longest <= 128 ? 8 : longest <= 256 ? 16 : longest <= 512 ? 32 : 64;
}
// aqc_capi_qc.hip, for aqc_create / aqc_destroy: the LDS the k-mer kernel may ask for; a context's k-mer tables freed
AQC_INTERNAL int allow_kmer_lds();
AQC_INTERNAL void free_kmer(KmerTable& t);
#ifdef AQC_PROFILE
AQC_INTERNAL void fetch_kprof(unsigned long long kp[16]);      // ... and the k-mer kernel's phase stamps, for aqc_get_counters
#endif

// how every entry point that takes (c, slot) begins: context and slot checked, the device current, `s` the slot
#define GET_SLOT(s)                      \
    Slot* s;                             \
    do {                                 \
        int rc_ = get_slot(c, slot, &s); \
        if (rc_) return rc_;             \
    } while (0)

}  // namespace aqc
