// aqc_capi.hip — host side of libafterqc_hip.so: the C ABI declared in include/afterqc_hip.h.
//
// One aqc_ctx per GPU.  Each slot owns a HIP stream, device copies of one batch (grow-on-demand,
// sized for 288 GB parts: batches of millions of pairs are the norm) and a result buffer; uploads
// are hipMemcpyAsync on the slot's stream so that slot k+1 uploads while slot k computes.
// Statistics (counters, histograms, QC accumulators, k-mer tables) live in HBM for the lifetime of
// the context and are only copied back on request.
//
// The C API is one translation unit per stage around aqc_ctx.hpp (the context, its slots, the helpers declared there):
//   aqc_capi.hip        this file: the error channel, the helpers' definitions, context and config, page-locked host memory,
//                       sync, timing, counters and histograms
//   aqc_capi_run.hip    upload, the verdict kernels, results, .gz out, the function seams, the libed.so pair
//   aqc_capi_qc.hip     statRead and the k-mer tables
//   aqc_capi_text.hip   text in, text out, the polyX census
// A device header that defines a non-template kernel is included by exactly one of them (the kernel would be defined twice
// otherwise); this unit includes none and launches no kernel.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <vector>

#include "aqc_ctx.hpp"
#include <sys/mman.h>
#include <sched.h>
#include <pthread.h>
#include <cctype>

using namespace aqc;

static thread_local char g_err[512] = "";

int aqc::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---- the helpers declared in aqc_ctx.hpp ---------------------------------------------------------------------------
namespace aqc {

// record the start/stop event of a launch: the "last launch" pair, or the next ring pair while collecting
hipEvent_t launch_event(Slot& s, int k, int which) {
    if (s.collecting && s.ring_used[k] < RING_CAP) {
        if ((int)s.ring[k][which].size() <= s.ring_used[k]) {
            hipEvent_t e = nullptr;
            (void)hipEventCreate(&e);
            s.ring[k][which].push_back(e);
        }
        hipEvent_t e = s.ring[k][which][s.ring_used[k]];
        if (which == 1) s.ring_used[k]++;
        return e;
    }
    return s.ev[k][which];
}

// everything queued for the slot has finished: its own stream and, if statRead kernels of this slot were sent to the
// context's QC stream, those too
hipError_t slot_sync(Slot& s) {
    hipError_t e = hipStreamSynchronize(s.stream);
    const uint64_t g = s.qc.gen.load(std::memory_order_acquire);
    if (e == hipSuccess && s.qc.synced.load(std::memory_order_acquire) < g) {
        e = hipEventSynchronize(s.ev_qc);          // (waits for the event's LATEST record: generation g or a newer one)
        if (e == hipSuccess) {
            uint64_t seen = s.qc.synced.load(std::memory_order_relaxed);
            while (seen < g && !s.qc.synced.compare_exchange_weak(seen, g, std::memory_order_release)) { }
        }
    }
    return e;
}

// what a status word says; the errors tied to a record (at_record) are upstream's exceptions inside its loop
const char* status_text(int st, bool at_record) {
    if (st == AQC_ERR_ALPHABET) return "a base outside the reference's COMP table reached the correction walk (KeyError upstream)";
    if (at_record) {
        if (st == AQC_ERR_INDEX) return "the overlap walk read a quality line beyond its length — the line is shorter than its sequence line (IndexError upstream)";
        if (st == AQC_ERR_ARG) return "a name field the bubble filter converts with int() is not a number (ValueError upstream)";
    } else {
        if (st == AQC_ERR_READ_TOO_LONG) return "a read (or its quality line) is longer than AQC_MAX_READ_LEN";
        if (st == AQC_ERR_ARG) return "a read shorter than 5 bases reached statRead (IndexError upstream)";
        if (st == AQC_ERR_UNSUPPORTED) return "device limit exceeded (k-mer table full or string longer than 64)";
    }
    return "device-side error";
}

int check_status(Slot& sl) {
    StatusWords w{0, 0, ~0ull};
    HIP_TRY(hipMemcpyAsync(&w, sl.status, sizeof(w), hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
    int st = w.status;
    if (st != 0) {
        (void)hipMemcpyAsync(sl.status, &STATUS_CLEAR, sizeof(STATUS_CLEAR), hipMemcpyHostToDevice, sl.stream);
        (void)hipStreamSynchronize(sl.stream);
        sl.err_record = UINT64_MAX;
        // (a hard device error raised first — a read beyond AQC_MAX_READ_LEN, a device limit — is reported as what it is: the records
        //  in front of a record-tied error are NOT valid then, and aqc_error_record stays unset; round-5 advisory)
        const bool record_kind = st == AQC_ERR_INDEX || st == AQC_ERR_ALPHABET || st == AQC_ERR_ARG;
        if (w.err_key != ~0ull && record_kind) {
            // an exception inside upstream's loop: the run ends at the EARLIEST record that raises, whatever raised first here
            sl.err_record = w.err_key >> 8;
            st = -(int)(w.err_key & 0xffu);
            return fail(st, "%s; record %llu of the chunk — the run ends there, the records before it are valid (aqc_error_record)", status_text(st, true),
                        (unsigned long long)sl.err_record);
        }
        return fail(st, "%s", status_text(st, false));
    }
    return 0;
}

int get_slot(aqc_ctx* c, int slot, Slot** out) {
    if (!c) return fail(AQC_ERR_ARG, "null context");
    if (slot < 0 || slot >= c->n_slots) return fail(AQC_ERR_ARG, "slot %d out of range", slot);
    HIP_TRY(hipSetDevice(c->device));
    *out = &c->slots[slot];
    return 0;
}

// the tail of a fetcher: `bytes` of the slot's device memory to the caller's `dst` (room for `cap`) on the slot's stream, the
// wait for them, and what the slot's kernels had to report
int fetch_out(Slot& s, const void* src, uint64_t bytes, void* dst, uint64_t cap, const char* who) {
    if (bytes > cap) return fail(AQC_ERR_ARG, "%s: %llu bytes do not fit %llu", who, (unsigned long long)bytes, (unsigned long long)cap);
    if (bytes) {
        if (!dst) return fail(AQC_ERR_ARG, "%s: null destination", who);
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s.stream));
    }
    HIP_TRY(hipStreamSynchronize(s.stream));
    return check_status(s);
}

// every slot of the context in sync, and what their kernels had to report: how the getters of the statistics begin
int sync_all(aqc_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    for (auto& s : c->slots) {
        HIP_TRY(slot_sync(s));
        int rc = check_status(s);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace aqc

extern "C" {

// ---- context and config ------------------------------------------------------------------------------------------
int aqc_abi_version(void) { return AQC_ABI_VERSION; }

int aqc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* aqc_last_error(void) { return g_err; }

int aqc_create(int device, int n_slots, aqc_ctx** out) {
    if (!out || n_slots < 1 || n_slots > 16) return fail(AQC_ERR_ARG, "aqc_create: bad arguments");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(AQC_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(AQC_ERR_ARG, "device %d out of range (%d visible)", device, n);
    HIP_TRY(hipSetDevice(device));
    {
        // host threads waiting for a stream sleep instead of spinning: the pipe keeps half a dozen of them in
        // hipStreamSynchronize, and under a CPU quota every spinning waiter is a core the gzip decoder does not get
        // (AQC_SYNC=spin keeps the runtime's default)
        const char* sy = getenv("AQC_SYNC");
        if (!(sy && !strcmp(sy, "spin")) && hipSetDeviceFlags(hipDeviceScheduleBlockingSync) != hipSuccess) (void)hipGetLastError();
    }
    aqc_ctx* c = new aqc_ctx();
    c->device = device;
    c->n_slots = n_slots;
    c->slots = std::vector<Slot>(n_slots);      // (built in place: a Slot owns its buffers and is never copied or moved)
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    snprintf(c->name, sizeof(c->name), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const char* fg = getenv("AQC_FORCE_GENERIC");
    c->force_generic = fg && fg[0] == '1';
    const char* fu = getenv("AQC_FUSED");
    c->fuse_opt = fu && fu[0] == '1';
    const char* qi = getenv("AQC_QC_STREAM");
    c->qc_inline = qi && qi[0] == '0';
    if (int rc = allow_kmer_lds()) return rc;
    HIP_TRY(hipStreamCreateWithFlags(&c->qc_stream, hipStreamNonBlocking));
    for (auto& s : c->slots) {
        HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        for (int k = 0; k < AQC_N_KERNELS; k++)
            for (int j = 0; j < 2; j++) HIP_TRY(hipEventCreate(&s.ev[k][j]));
        HIP_TRY(hipEventCreateWithFlags(&s.ev_main, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.ev_qc, hipEventDisableTiming));
    }
    HIP_TRY(hipMalloc((void**)&c->counters, sizeof(unsigned long long) * (AQC_N_COUNTERS + 16)));   // +16: AQC_PROFILE builds
    HIP_TRY(hipMalloc((void**)&c->ovl_hist, sizeof(unsigned long long) * AQC_QC_COLS));
    HIP_TRY(hipMalloc((void**)&c->dist_hist, sizeof(unsigned long long) * AQC_QC_COLS));
    for (auto& s : c->slots) {
        HIP_TRY(hipMalloc((void**)&s.status, sizeof(StatusWords)));
        HIP_TRY(hipMemcpy(s.status, &STATUS_CLEAR, sizeof(STATUS_CLEAR), hipMemcpyHostToDevice));
    }
    for (int k = 0; k < 4; k++)
        HIP_TRY(hipMalloc((void**)&c->qc[k].acc, sizeof(unsigned long long) * AQC_QC_ROWS * AQC_QC_COLS));
    *out = c;
    return aqc_reset_stats(c);
}

void aqc_destroy(aqc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto& s : c->slots) {
        for (int k = 0; k < AQC_N_KERNELS; k++)
            for (int j = 0; j < 2; j++) {
                if (s.ev[k][j]) (void)hipEventDestroy(s.ev[k][j]);
                for (hipEvent_t e : s.ring[k][j]) (void)hipEventDestroy(e);
            }
        if (s.status) (void)hipFree(s.status);
        for (hipEvent_t e : s.census_ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : s.adp_census_ev) if (e) (void)hipEventDestroy(e);
        for (ViewPass& vp : s.pass)
            for (hipEvent_t e : vp.ev) if (e) (void)hipEventDestroy(e);
        if (s.ev_main) (void)hipEventDestroy(s.ev_main);
        if (s.ev_qc) (void)hipEventDestroy(s.ev_qc);
        if (s.stream) (void)hipStreamDestroy(s.stream);
    }
    if (c->qc_stream) (void)hipStreamDestroy(c->qc_stream);
    (void)hipFree(c->counters); (void)hipFree(c->ovl_hist); (void)hipFree(c->dist_hist);
    for (PassCounts& pc : c->pass_stats) pc.free();
    for (AdpCensus& ac : c->adp_census) ac.free();
    for (int k = 0; k < 4; k++) {
        (void)hipFree(c->qc[k].acc);
        free_kmer(c->qc[k].kt);
    }
    delete c;      // (every DevBuf of the context and its slots goes here, with their device current)
}

int aqc_device_index(aqc_ctx* c) { return c ? c->device : -1; }

// The NUMA node the GPU hangs off (its PCI function's numa_node in sysfs); -1: unknown / the host has a single node.
int aqc_device_numa_node_of(int device) {
    char bus[64] = "";
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char* p = bus; *p; ++p) *p = (char)tolower((unsigned char)*p);
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    int node = -1;
    if (FILE* f = fopen(path, "r")) {
        if (fscanf(f, "%d", &node) != 1) node = -1;
        fclose(f);
    }
    return node;
}
int aqc_device_numa_node(aqc_ctx* c) { return c ? aqc_device_numa_node_of(c->device) : -1; }

// Bind the calling thread to the CPUs of `node` that it may run on (its current affinity mask intersected with the node's
// cpulist); memory the thread touches first then comes from that node.  Returns the number of CPUs it is bound to, 0 when
// nothing was changed (unknown node, a single-node host, an empty intersection, AQC_PIPE_NUMA=0).
int aqc_bind_thread_to_node(int node) {
    if (node < 0) return 0;
    if (const char* e = getenv("AQC_PIPE_NUMA")) if (e[0] == '0') return 0;
    char path[96];
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r");
    if (!f) return 0;
    char list[4096] = "";
    const bool got = fgets(list, sizeof(list), f) != nullptr;
    fclose(f);
    if (!got) return 0;
    cpu_set_t have, want;
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(have), &have) != 0) return 0;
    int n = 0;
    for (char* p = list; *p;) {
        char* q;
        const long a = strtol(p, &q, 10);
        if (q == p) break;
        long b = a;
        if (*q == '-') { p = q + 1; b = strtol(p, &q, 10); }
        for (long cpu = a; cpu <= b && cpu < CPU_SETSIZE; ++cpu)
            if (CPU_ISSET((int)cpu, &have)) { CPU_SET((int)cpu, &want); ++n; }
        p = *q == ',' ? q + 1 : q;
        if (*q != ',') break;
    }
    if (n == 0 || n == CPU_COUNT(&have)) return 0;           // nothing to choose from
    if (pthread_setaffinity_np(pthread_self(), sizeof(want), &want) != 0) return 0;
    return n;
}

int aqc_device_name(aqc_ctx* c, char* buf, int buflen) {
    if (!c || !buf || buflen <= 0) return fail(AQC_ERR_ARG, "aqc_device_name: bad arguments");
    snprintf(buf, (size_t)buflen, "%s", c->name);
    return 0;
}

int aqc_set_config(aqc_ctx* c, const aqc_config* cfg) {
    if (!c || !cfg) return fail(AQC_ERR_ARG, "aqc_set_config: null argument");
    if (cfg->trim_front < 0 || cfg->trim_tail < 0 || cfg->trim_front2 < 0 || cfg->trim_tail2 < 0)
        return fail(AQC_ERR_ARG, "trim values must be resolved (>= 0) before they reach the device");
    if (cfg->qc_kmer < 1 || cfg->qc_kmer > 8) return fail(AQC_ERR_UNSUPPORTED, "qc_kmer %d outside 1..8", cfg->qc_kmer);
    if (cfg->barcode) {
        if (cfg->barcode_verify_len < 0 || cfg->barcode_verify_len > 32 || cfg->barcode_length < 1 ||
            cfg->barcode_length + 1 + cfg->barcode_verify_len > 62)
            return fail(AQC_ERR_UNSUPPORTED, "barcode_length + verify too long for the device path");
    }
    c->cfg = *cfg;
    c->has_cfg = true;
    return 0;
}

// the quality cut (aqc_qcut.hpp): NULL or no mode set switches it off
int aqc_set_quality_cut(aqc_ctx* c, const aqc_cut_config* cut) {
    if (!c) return fail(AQC_ERR_ARG, "aqc_set_quality_cut: null context");
    QcutOpts o{};
    if (cut) o = QcutOpts{cut->front ? 1 : 0, cut->tail ? 1 : 0, cut->right ? 1 : 0, cut->window, cut->mean_quality};
    if (!qcut_on(o)) { c->cut = QcutOpts{}; return 0; }
    if (!qcut_opts_ok(o))
        return fail(AQC_ERR_ARG, "aqc_set_quality_cut: window %d (1 .. %d) / mean quality %d (0 .. %d)", o.window, AQC_MAX_READ_LEN, o.mean_quality, QCUT_MAX_QUALITY);
    HIP_TRY(c->pass_stats[VP_CUT].ensure(c->device));
    c->cut = o;
    return 0;
}

// the four counts of a view pass, once every slot's work is done
static int get_pass_stats(aqc_ctx* c, ViewPassId which, int64_t out[4]) {
    if (!c || !out) return fail(AQC_ERR_ARG, "null argument");
    int rc = sync_all(c);
    if (rc) return rc;
    HIP_TRY(c->pass_stats[which].get(out));
    return 0;
}
int aqc_get_cut_stats(aqc_ctx* c, int64_t out[4]) { return get_pass_stats(c, VP_CUT, out); }

// the adapters to trim (aqc_adapter.hpp): NULL or both lengths 0 switches the pass off
int aqc_set_adapter_trim(aqc_ctx* c, const aqc_adapter_config* adapter) {
    if (!c) return fail(AQC_ERR_ARG, "aqc_set_adapter_trim: null context");
    AdapterOpts a{};
    if (!adp_from_config(adapter, a))
        return fail(AQC_ERR_ARG, "aqc_set_adapter_trim: adapter lengths %d / %d (0 or %d .. %d letters of ACGT), min overlap %d (1 .. the shorter adapter)",
                    adapter->len1, adapter->len2, ADP_MIN_LEN, ADP_MAX_LEN, adapter->min_overlap);
    if (!adp_on(a)) { c->adapter = AdapterOpts{}; return 0; }
    HIP_TRY(c->pass_stats[VP_ADAPTER].ensure(c->device));
    c->adapter = a;
    return 0;
}

int aqc_get_adapter_stats(aqc_ctx* c, int64_t out[4]) { return get_pass_stats(c, VP_ADAPTER, out); }

// the letters whose tails are cut (aqc_polytail.hpp): NULL or every length 0 switches the pass off
int aqc_set_poly_trim(aqc_ctx* c, const aqc_poly_config* poly) {
    if (!c) return fail(AQC_ERR_ARG, "aqc_set_poly_trim: null context");
    PolyOpts o{};
    if (!poly_from_config(poly, o))
        return fail(AQC_ERR_ARG, "aqc_set_poly_trim: minimum lengths %d / %d / %d / %d of A / C / G / T (0: off, or 1 .. %d)", poly->min_len[0], poly->min_len[1],
                    poly->min_len[2], poly->min_len[3], POLY_MAX_MIN_LEN);
    if (!poly_on(o)) { c->poly = PolyOpts{}; return 0; }
    HIP_TRY(c->pass_stats[VP_POLY].ensure(c->device));
    c->poly = o;
    return 0;
}

int aqc_get_poly_stats(aqc_ctx* c, int64_t out[4]) { return get_pass_stats(c, VP_POLY, out); }

int aqc_set_circles(aqc_ctx* c, const double* cx, const double* cy, const double* r, const int32_t* lane,
                    const int32_t* tile, int32_t n) {
    if (!c || n < 0) return fail(AQC_ERR_ARG, "aqc_set_circles: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    c->circles = DevCircles{};
    c->circles.n = n;
    if (n == 0) return 0;
    const void* src[5] = {cx, cy, r, lane, tile};
    const size_t sz[5] = {sizeof(double) * n, sizeof(double) * n, sizeof(double) * n, sizeof(int32_t) * n, sizeof(int32_t) * n};
    for (int k = 0; k < 5; k++) {
        if (!src[k]) return fail(AQC_ERR_ARG, "aqc_set_circles: null array");
        if (c->circ[k].reserve(sz[k])) return fail(AQC_ERR_HIP, "hipMalloc failed");
        HIP_TRY(hipMemcpy(c->circ[k].p, src[k], sz[k], hipMemcpyHostToDevice));
    }
    c->circles.cx = (const double*)c->circ[0].p;
    c->circles.cy = (const double*)c->circ[1].p;
    c->circles.cr = (const double*)c->circ[2].p;
    c->circles.lane = (const int32_t*)c->circ[3].p;
    c->circles.tile = (const int32_t*)c->circ[4].p;
    return 0;
}

int aqc_reset_stats(aqc_ctx* c) {
    if (!c) return fail(AQC_ERR_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(c->counters, 0, sizeof(unsigned long long) * (AQC_N_COUNTERS + 16)));
    HIP_TRY(hipMemset(c->ovl_hist, 0, sizeof(unsigned long long) * AQC_QC_COLS));
    HIP_TRY(hipMemset(c->dist_hist, 0, sizeof(unsigned long long) * AQC_QC_COLS));
    for (PassCounts& pc : c->pass_stats) HIP_TRY(pc.zero());
    for (AdpCensus& ac : c->adp_census) HIP_TRY(ac.zero());
    for (auto& sl : c->slots) { HIP_TRY(hipMemcpy(sl.status, &STATUS_CLEAR, sizeof(STATUS_CLEAR), hipMemcpyHostToDevice)); sl.err_record = UINT64_MAX; }
    for (int k = 0; k < 4; k++) {
        HIP_TRY(hipMemset(c->qc[k].acc, 0, sizeof(unsigned long long) * AQC_QC_ROWS * AQC_QC_COLS));
        c->qc[k].last_end = 0;
        c->qc[k].epoch = 0;
        if (c->qc[k].kt.keys) {
            HIP_TRY(hipMemset(c->qc[k].kt.keys, 0, sizeof(unsigned long long) * KMER_CAP));
            HIP_TRY(hipMemset(c->qc[k].kt.counts, 0, sizeof(unsigned long long) * (KMER_CAP + 1)));
            HIP_TRY(hipMemset(c->qc[k].kt.order, 0xff, sizeof(unsigned long long) * (KMER_CAP + 1)));
            HIP_TRY(hipMemset(c->qc[k].kt.dense_count, 0, sizeof(unsigned int) * DENSE_CAP));
            HIP_TRY(hipMemset(c->qc[k].kt.dense_first, 0xff, sizeof(unsigned long long) * DENSE_CAP));
            HIP_TRY(hipMemset(c->qc[k].kt.complete, 0, sizeof(unsigned int) * (DENSE_ENTRIES / KRED_ENTRIES)));
        }
    }
    HIP_TRY(hipDeviceSynchronize());   // (non-blocking slot streams do not wait for the null stream)
    return 0;
}

// ---- page-locked host memory -------------------------------------------------------------------------------------
// Page-locked host memory.  Not hipHostMalloc: in a fresh process that costs 0.17 s per GiB (4 KiB pages faulted and pinned one by
// one, and calls from several threads serialise), which is as long as the whole 10 M-read job takes.  Anonymous memory on
// transparent huge pages, touched and then registered, is the same memory to the DMA engines (56.7 GB/s H2D either way) for
// 0.04 s per GiB, and threads do it side by side (tools/ubench/pin_rate.cpp).  Portable: the rings are filled by reader threads
// under whichever device is current and DMA-ed from by any context.
// (an unnamed namespace INSIDE the extern "C" block: g_host_mu and g_host_regions are in the library's dynamic symbol table
//  under these C names, and that table is kept as it is)
namespace {
struct HostRegion { void* user; void* base; size_t map_len; bool registered; };
std::mutex g_host_mu;
std::vector<HostRegion> g_host_regions;
}  // namespace

void* aqc_host_alloc(uint64_t bytes) {
    const size_t HUGE = 2u << 20;
    const size_t len = (((size_t)(bytes ? bytes : 1)) + HUGE - 1) & ~(HUGE - 1);
    void* base = bytes >= (1u << 20) ? mmap(nullptr, len + HUGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0) : MAP_FAILED;
    if (base != MAP_FAILED) {
        uint8_t* p = (uint8_t*)(((uintptr_t)base + HUGE - 1) & ~(uintptr_t)(HUGE - 1));
        (void)madvise(p, len, MADV_HUGEPAGE);
        for (size_t o = 0; o < len; o += 4096) ((volatile uint8_t*)p)[o] = 0;
        if (hipHostRegister(p, len, hipHostRegisterPortable) == hipSuccess) {
            std::lock_guard<std::mutex> g(g_host_mu);
            g_host_regions.push_back(HostRegion{p, base, len + HUGE, true});
            return p;
        }
        (void)hipGetLastError();
        munmap(base, len + HUGE);
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) return nullptr;
    return p;
}

void aqc_host_free(void* p) {
    if (!p) return;
    HostRegion r{nullptr, nullptr, 0, false};
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        for (size_t i = 0; i < g_host_regions.size(); ++i)
            if (g_host_regions[i].user == p) { r = g_host_regions[i]; g_host_regions.erase(g_host_regions.begin() + (long)i); break; }
    }
    if (r.registered) {
        (void)hipHostUnregister(r.user);
        munmap(r.base, r.map_len);
    } else (void)hipHostFree(p);
}

// ---- sync, timing -----------------------------------------------------------------------------------------------
int aqc_sync(aqc_ctx* c, int slot) {
    GET_SLOT(s);
    HIP_TRY(slot_sync(*s));
    return check_status(*s);
}

int aqc_error_record(aqc_ctx* c, int slot, uint64_t* record) {
    GET_SLOT(s);
    if (!record) return fail(AQC_ERR_ARG, "aqc_error_record: null argument");
    *record = s->err_record;
    return 0;
}

int aqc_kernel_ms(aqc_ctx* c, int slot, float* ms) {
    GET_SLOT(s);
    HIP_TRY(slot_sync(*s));
    for (int k = 0; k < AQC_N_KERNELS; k++) {
        ms[k] = 0.f;
        if (s->timed[k]) HIP_TRY(hipEventElapsedTime(&ms[k], s->ev[k][0], s->ev[k][1]));
    }
    return 0;
}

int aqc_timing_reset(aqc_ctx* c, int slot) {
    GET_SLOT(s);
    HIP_TRY(slot_sync(*s));
    for (int k = 0; k < AQC_N_KERNELS; k++) { s->ring_used[k] = 0; s->timed[k] = false; }
    s->collecting = true;
    return 0;
}

int aqc_timing_mean(aqc_ctx* c, int slot, float* mean_ms, int32_t* launches) {
    GET_SLOT(s);
    if (!mean_ms || !launches) return fail(AQC_ERR_ARG, "null argument");
    HIP_TRY(slot_sync(*s));
    for (int k = 0; k < AQC_N_KERNELS; k++) {
        double sum = 0;
        for (int i = 0; i < s->ring_used[k]; i++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, s->ring[k][0][i], s->ring[k][1][i]));
            sum += ms;
        }
        launches[k] = s->ring_used[k];
        mean_ms[k] = s->ring_used[k] ? (float)(sum / s->ring_used[k]) : 0.f;
    }
    s->collecting = false;
    return 0;
}

// ---- counters and QC getters -------------------------------------------------------------------------------------
int aqc_get_counters(aqc_ctx* c, int64_t* out) {
    if (!c || !out) return fail(AQC_ERR_ARG, "null argument");
    int rc = sync_all(c);
    if (rc) return rc;
#ifdef AQC_PROFILE
    {
        unsigned long long pr[16];
        (void)hipMemcpy(pr, c->counters + AQC_N_COUNTERS, sizeof(pr), hipMemcpyDeviceToHost);
        unsigned long long tot = 0;
        for (int k = 0; k < 10; k++) tot += pr[k];
        static const char* nm[10] = {"phase1", "normalise", "bubble+len+polyX", "lowq+N", "scan", "verify", "post+walk", "results+counters", "deferred", "-"};
        for (int k = 0; k < 9; k++) fprintf(stderr, "PROF %-18s %6.2f %%\n", nm[k], tot ? 100.0 * pr[k] / tot : 0.0);
        fprintf(stderr, "DEFER alphabet/length %llu  short-partner %llu  adapter-second-scan %llu  walk-anchor %llu\n", pr[10], pr[11], pr[12], pr[13]);
        // load balance of the last fast-kernel launch of slot 0: spread of the waves' end stamps
        {
            Slot& s0 = c->slots[0];
            if (s0.used_fast && s0.n > (1u << 16) && s0.deferred.p) {
                const size_t nw = 4096;
                std::vector<uint32_t> st(2 * nw);
                (void)hipMemcpy(st.data(), (uint32_t*)s0.deferred.p + (s0.n - 2 * nw), sizeof(uint32_t) * 2 * nw, hipMemcpyDeviceToHost);
                // (s_memtime runs on the shader clock and is not synchronised across XCDs: only lifetimes are meaningful)
                std::vector<uint32_t> life;
                double sum_life = 0;
                for (size_t w = 0; w < nw; ++w) { const uint32_t d = st[2 * w + 1] - st[2 * w]; life.push_back(d); sum_life += d; }
                {
                    // by XCD (workgroups are dealt round-robin to the 8 XCDs) and by position in the grid
                    double xs[8] = {0}, qs[4] = {0};
                    for (size_t w = 0; w < nw; ++w) {
                        const size_t gw = nw - 1 - w;          // stamps are stored from the tail backwards
                        xs[(gw / 4) % 8] += life[w];
                        qs[gw * 4 / nw] += life[w];
                    }
                    fprintf(stderr, "WAVES mean lifetime by XCD:");
                    for (int x = 0; x < 8; ++x) fprintf(stderr, " %.0f", xs[x] / (nw / 8));
                    fprintf(stderr, "  by grid quarter:");
                    for (int q = 0; q < 4; ++q) fprintf(stderr, " %.0f", qs[q] / (nw / 4));
                    fprintf(stderr, "\n");
                }
                std::sort(life.begin(), life.end());
                fprintf(stderr, "WAVES lifetime in shader clocks: min %u p10 %u median %u p90 %u max %u mean %.0f\n", life.front(), life[nw / 10],
                        life[nw / 2], life[nw * 9 / 10], life.back(), sum_life / nw);
            }
        }
        unsigned long long kp[16];
        fetch_kprof(kp);
        tot = 0;
        for (int k = 0; k < 8; k++) tot += kp[k];
        static const char* kn[8] = {"zero+sync", "descriptors", "front(ws,shfl)", "lds adds", "first-seen", "exotic", "round-end sync", "writeout"};
        for (int k = 0; k < 8; k++) fprintf(stderr, "KPROF %-16s %6.2f %%\n", kn[k], tot ? 100.0 * kp[k] / tot : 0.0);
    }
#endif
    HIP_TRY(hipMemcpy(out, c->counters, sizeof(int64_t) * AQC_N_COUNTERS, hipMemcpyDeviceToHost));
    return 0;
}

int aqc_get_histograms(aqc_ctx* c, int64_t* ovl, int64_t* dist, int32_t n) {
    if (!c || !ovl || !dist || n < 0 || n > AQC_QC_COLS) return fail(AQC_ERR_ARG, "bad argument");
    int rc = sync_all(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(ovl, c->ovl_hist, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dist, c->dist_hist, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
