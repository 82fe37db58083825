// aqc_capi_qc.hip — the C API's statRead stage: the k-mer tables of a context (built on first use, freed with it), aqc_qc_stat, and
// the getters of what it accumulates (aqc_get_qc, aqc_get_kmers); and the second census of the same pass-1 sample, the adapter
// census (aqc_set_adapter_probes, aqc_adapter_census and its getters).  The context, its slots and the shared helpers: aqc_ctx.hpp.
//
// Kernels launched here, and nowhere else (this is the one unit that includes aqc_qcstat.hpp, and the one that instantiates
// aqc_adpcensus.hpp's kernel):
//   qc_stat_kernel, kmer_count_kernel, kmer_reduce_kernel, kmer_compact_kernel, kmer_compact_dense_kernel, adapter_census_kernel<G>
#include <hip/hip_runtime.h>

#include <mutex>

#include "aqc_ctx.hpp"
#include "aqc_prim.hpp"
#include "aqc_qcstat.hpp"

using namespace aqc;

// ---- what aqc_capi.hip needs of this unit (declared in aqc_ctx.hpp) ----------------------------------------------
namespace aqc {

// the fused k-mer kernel asks for more dynamic LDS than a launch gets by default (aqc_create)
int allow_kmer_lds() {
    HIP_TRY(hipFuncSetAttribute((const void*)kmer_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KMER_FUSED_LDS_BYTES));
    return 0;
}

void free_kmer(KmerTable& t) {
    (void)hipFree(t.keys); (void)hipFree(t.counts); (void)hipFree(t.order);
    (void)hipFree(t.dense_count); (void)hipFree(t.dense_first); (void)hipFree(t.complete);
    t = KmerTable{};
}

#ifdef AQC_PROFILE
void fetch_kprof(unsigned long long kp[16]) { (void)hipMemcpyFromSymbol(kp, HIP_SYMBOL(g_kprof), 16 * sizeof(unsigned long long)); }
#endif

}  // namespace aqc

extern "C" {

// ---- statRead ----------------------------------------------------------------------------------------------------
static int kmer_array(void** p, size_t bytes, int fill) {
    HIP_TRY(hipMalloc(p, bytes));
    HIP_TRY(hipMemset(*p, fill, bytes));
    return 0;
}

static int build_kmer(KmerTable& t) {
    int rc;
    if ((rc = kmer_array((void**)&t.keys, sizeof(unsigned long long) * KMER_CAP, 0)) ||
        (rc = kmer_array((void**)&t.counts, sizeof(unsigned long long) * (KMER_CAP + 1), 0)) ||      // (+1: the all-NUL k-mer, see kmer_slot)
        (rc = kmer_array((void**)&t.order, sizeof(unsigned long long) * (KMER_CAP + 1), 0xff)) ||
        (rc = kmer_array((void**)&t.dense_count, sizeof(unsigned int) * DENSE_CAP, 0)) ||
        (rc = kmer_array((void**)&t.dense_first, sizeof(unsigned long long) * DENSE_CAP, 0xff)) ||
        (rc = kmer_array((void**)&t.complete, sizeof(unsigned int) * (DENSE_ENTRIES / KRED_ENTRIES), 0)))
        return rc;
    t.mask = KMER_CAP - 1;
    // the slot streams are non-blocking: make sure the fills have landed before any kernel can touch the tables
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// (the context sees a table only once all of it exists: a set-up that failed half way leaves q.kt empty, and the next call tries again)
static int ensure_kmer(QcDev& q) {
    if (q.kt.keys) return 0;
    KmerTable t{};
    const int rc = build_kmer(t);
    if (rc) free_kmer(t);
    else q.kt = t;
    return rc;
}

int aqc_qc_stat(aqc_ctx* c, int slot, int which, int mate, uint64_t first, uint64_t count, int post) {
    GET_SLOT(s);
    int rc;
    if (which < 0 || which > 3 || mate < 0 || mate > 1) return fail(AQC_ERR_ARG, "aqc_qc_stat: bad which/mate");
    if (!c->has_cfg) return fail(AQC_ERR_STATE, "aqc_qc_stat before aqc_set_config");
    if (first + count > s->n) return fail(AQC_ERR_ARG, "aqc_qc_stat: range exceeds the slot's %llu records", (unsigned long long)s->n);
    if (mate == 1 && !s->paired) return fail(AQC_ERR_ARG, "aqc_qc_stat: mate 1 of a single-end slot");
    if (post && !s->ran) return fail(AQC_ERR_STATE, "aqc_qc_stat(post) before aqc_run");
    if (count == 0) return 0;
    // one call at a time per context: the count -> reduce pairs below go through ONE slice buffer (kmer_partial) in stream order
    std::lock_guard<std::mutex> qc_lock(c->qc_mu);
    QcDev& q = c->qc[which];
    if ((rc = ensure_kmer(q))) return rc;
    // the statRead kernels go to the context's QC stream, behind everything queued on the slot's stream so far (text, results):
    // a few thousand latency-bound waves that overlap with the slot's bandwidth-bound kernels (the formatter) instead of
    // holding them up.  The slot is "in sync" again only when they are done too (slot_sync).
    // (AQC_QC_STREAM=0: on the slot's own stream, one kernel after the other — for profiles: beside the formatter a statRead kernel's
    //  start-to-end time is mostly the wait for free wave slots, e.g. 1.38 ms for a kernel whose waves live 0.06 ms)
    hipStream_t qs = c->qc_inline ? s->stream : c->qc_stream;
    HIP_TRY(hipEventRecord(s->ev_main, s->stream));
    if (!c->qc_inline) HIP_TRY(hipStreamWaitEvent(qs, s->ev_main, 0));
    HIP_TRY(hipEventRecord(launch_event(*s, AQC_K_QC_STAT, 0), qs));
    // LDS sized by the longest read of the slot: many resident workgroups for short reads
    const uint32_t mx = s->raw_max_len ? s->raw_max_len : AQC_MAX_READ_LEN;
    int cols = (int)((mx + 63) / 64 * 64);
    if (cols > AQC_QC_COLS) cols = AQC_QC_COLS;
    const size_t lds = sizeof(unsigned int) * (size_t)(QC_LDS_ROWS + 1) * cols + 16;
    // two 1024-thread workgroups per CU (every wave slot taken) and as few workgroups as that allows: each one ends
    // with ~11 global atomics per cycle; more only when a workgroup's packed counters would pass 4095 reads
    uint64_t blocks = (count + QC_WPB - 1) / QC_WPB;
    if (blocks > (uint64_t)c->n_cu * 2) blocks = (uint64_t)c->n_cu * 2;
    const uint64_t need = (count + (QC_MAX_READS_PER_BLOCK - QC_WPB) - 1) / (QC_MAX_READS_PER_BLOCK - QC_WPB);
    if (blocks < need) blocks = need;
    const unsigned long long g0 = s->view.first_index + first;
    if (g0 < q.last_end) q.epoch++;
    q.last_end = g0 + count;
    const unsigned long long order_base = (q.epoch << 34) | g0;
    // Reads of <= 256 bases: ONE kernel does both halves of statRead (per-cycle rows ride along with the k-mer
    // counting, see kmer_count_kernel); longer reads: the per-cycle kernel runs on its own.
    const uint32_t per_read = mx > (uint32_t)c->cfg.qc_kmer ? mx - (uint32_t)c->cfg.qc_kmer : 1;
    uint32_t rpr_max = 65535u / per_read;
    if (rpr_max < 1) rpr_max = 1;
    const uint64_t max_rounds = 512;                       // 64 MiB of slices at most per launch
    const uint64_t rounds_per_block = (max_rounds + c->n_cu - 1) / c->n_cu;
    const bool fused = cols <= KMER_FUSED_MAX_COLS && rounds_per_block * rpr_max <= (uint64_t)QC_MAX_READS_PER_BLOCK;
    // (fused: the reads whose quality line has a length of its own — a slot that has any: s->has_irregular — get their per-cycle rows
    //  from this kernel too, and only those; their k-mers are counted with everybody else's)
    if (!fused || s->has_irregular)
        hipLaunchKernelGGL(qc_stat_kernel, dim3((unsigned)blocks), dim3(QC_BLOCK), lds, qs, s->view, mate, first, count, post,
                           (const aqc_result*)s->results.p, c->cfg.qc_kmer, q.acc, s->status, cols, fused ? 1 : 0);
    // k-mer dictionary: LDS-resident u16 counters, rounds of <= 65535 k-mers per workgroup, slices reduced afterwards
    {
        uint64_t done = 0;
        while (done < count) {
            uint64_t chunk = count - done;
            if (chunk > max_rounds * rpr_max) chunk = max_rounds * rpr_max;
            // every workgroup the same number of rounds: round the count up to a multiple of the CU count
            uint64_t n_rounds64 = (chunk + rpr_max - 1) / rpr_max;
            if (n_rounds64 > (uint64_t)c->n_cu) {
                n_rounds64 = (n_rounds64 + c->n_cu - 1) / c->n_cu * c->n_cu;
                if (n_rounds64 > max_rounds) n_rounds64 = max_rounds;
            }
            const uint32_t rpr = (uint32_t)((chunk + n_rounds64 - 1) / n_rounds64);
            const uint32_t n_rounds = (uint32_t)((chunk + rpr - 1) / rpr);
            if (c->kmer_partial.reserve((size_t)n_rounds * DENSE_ENTRIES * sizeof(uint16_t))) return fail(AQC_ERR_HIP, "hipMalloc failed");
            unsigned kb = n_rounds < (unsigned)c->n_cu ? n_rounds : (unsigned)c->n_cu;
            hipLaunchKernelGGL(kmer_count_kernel, dim3(kb), dim3(KMER_BLOCK), fused ? KMER_FUSED_LDS_BYTES : KMER_LDS_BYTES, qs, s->view,
                               mate, first + done, chunk, post, (const aqc_result*)s->results.p, c->cfg.qc_kmer, q.kt, order_base + done,
                               (uint16_t*)c->kmer_partial.p, rpr, n_rounds, s->status, fused ? q.acc : (unsigned long long*)nullptr,
                               fused ? cols : 0);
            hipLaunchKernelGGL(kmer_reduce_kernel, dim3(DENSE_ENTRIES / KRED_ENTRIES), dim3(KRED_BLOCK), 0, qs,
                               (const uint16_t*)c->kmer_partial.p, n_rounds, q.kt, c->cfg.qc_kmer);
            done += chunk;
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(launch_event(*s, AQC_K_QC_STAT, 1), qs));
    HIP_TRY(hipEventRecord(s->ev_qc, qs));
    s->qc.gen.fetch_add(1, std::memory_order_release);
    s->timed[AQC_K_QC_STAT] = !s->collecting;
    return 0;
}

// ---- QC getters --------------------------------------------------------------------------------------------------
int aqc_get_qc(aqc_ctx* c, int which, int64_t* out) {
    if (!c || !out || which < 0 || which > 3) return fail(AQC_ERR_ARG, "bad argument");
    int rc = sync_all(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, c->qc[which].acc, sizeof(int64_t) * AQC_QC_ROWS * AQC_QC_COLS, hipMemcpyDeviceToHost));
    return 0;
}

int aqc_get_kmers(aqc_ctx* c, int which, uint64_t* keys, int64_t* counts, uint64_t* order, uint64_t cap, uint64_t* n) {
    if (!c || !n || which < 0 || which > 3) return fail(AQC_ERR_ARG, "bad argument");
    int rc = sync_all(c);
    if (rc) return rc;
    *n = 0;
    QcDev& q = c->qc[which];
    if (!q.kt.keys) return 0;
    const uint64_t dcap = cap < KMER_CAP + 1 + DENSE_CAP ? cap : KMER_CAP + 1 + DENSE_CAP;
    DevBuf dk, dc, dord, dn;
    if (dk.reserve(8 * (dcap + 1)) || dc.reserve(8 * (dcap + 1)) || dord.reserve(8 * (dcap + 1)) || dn.reserve(8)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemset(dn.p, 0, 8));
    hipLaunchKernelGGL(kmer_compact_kernel, dim3((unsigned)(KMER_CAP / 256 + 1)), dim3(256), 0, 0, q.kt, (unsigned long long*)dk.p, (unsigned long long*)dc.p,
                       (unsigned long long*)dord.p, (unsigned long long)dcap, (unsigned long long*)dn.p);
    hipLaunchKernelGGL(kmer_compact_dense_kernel, dim3((unsigned)(DENSE_ENTRIES / 256)), dim3(256), 0, 0, q.kt, c->cfg.qc_kmer, (unsigned long long*)dk.p,
                       (unsigned long long*)dc.p, (unsigned long long*)dord.p, (unsigned long long)dcap, (unsigned long long*)dn.p);
    HIP_TRY(hipGetLastError());
    unsigned long long m = 0;
    HIP_TRY(hipMemcpy(&m, dn.p, 8, hipMemcpyDeviceToHost));
    const uint64_t w = m < dcap ? m : dcap;
    if (w) {
        HIP_TRY(hipMemcpy(keys, dk.p, 8 * w, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(counts, dc.p, 8 * w, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(order, dord.p, 8 * w, hipMemcpyDeviceToHost));
    }
    *n = m;
    if (m > dcap) return fail(AQC_ERR_ARG, "aqc_get_kmers: %llu entries exceed cap %llu", m, (unsigned long long)dcap);
    return 0;
}

// ---- the adapter census (aqc_adpcensus.hpp) ----------------------------------------------------------------------------
static_assert(AQC_ADP_PROBE_LEN == CEN_PROBE_LEN && AQC_ADP_MAX_PROBES == CEN_MAX_PROBES, "the C API's probes fill the kernel's");

static bool census_which(int which) { return which == AQC_QC_R1_PRE || which == AQC_QC_R2_PRE; }

// the probes of one pre-filter file (NULL: off); the file's counts start at zero
int aqc_set_adapter_probes(aqc_ctx* c, int which, const aqc_adapter_probes* probes) {
    if (!c || !census_which(which)) return fail(AQC_ERR_ARG, "aqc_set_adapter_probes: null context or `which` is no pre-filter file");
    AdpCensus& ac = c->adp_census[which];
    CensusProbes p{};
    if (probes && !cen_from_letters(probes->n, probes->seq, p))
        return fail(AQC_ERR_ARG, "aqc_set_adapter_probes: %d probes (1 .. %d, each %d letters of ACGT)", probes->n, CEN_MAX_PROBES, CEN_PROBE_LEN);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());                 // (a census of the probes that go may still count)
    if (probes) HIP_TRY(ac.ensure(c->device));
    HIP_TRY(ac.zero());
    ac.probes = p;
    return 0;
}

int aqc_adapter_census(aqc_ctx* c, int slot, int which, int mate, uint64_t first, uint64_t count) {
    GET_SLOT(s);
    if (!census_which(which) || mate < 0 || mate > 1) return fail(AQC_ERR_ARG, "aqc_adapter_census: bad which/mate");
    AdpCensus& ac = c->adp_census[which];
    if (ac.probes.n == 0) return fail(AQC_ERR_STATE, "aqc_adapter_census before aqc_set_adapter_probes");
    if (first > s->n || count > s->n - first) return fail(AQC_ERR_ARG, "aqc_adapter_census: range exceeds the slot's %llu records", (unsigned long long)s->n);
    if (mate == 1 && !s->paired) return fail(AQC_ERR_ARG, "aqc_adapter_census: mate 1 of a single-end slot");
    s->adp_census_ran = false;
    if (count == 0) return 0;
    // on the slot's own stream, behind what filled it: the statRead kernels of the same records run beside it on the QC stream
    CensusArgs A{};
    A.seq = mate ? s->view.seq2 : s->view.seq1; A.off = mate ? s->view.off2 : s->view.off1; A.len = mate ? s->view.len2 : s->view.len1;
    A.first = first; A.count = count; A.acc = ac.acc; A.status = s->status; A.probes = ac.probes;
    for (hipEvent_t& e : s->adp_census_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(s->adp_census_ev[0], s->stream));
    vp_dispatch(view_pass_lanes(*s), count, c->n_cu, [&](auto G, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(adapter_census_kernel<decltype(G)::value>, grid, block, 0, s->stream, A);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->adp_census_ev[1], s->stream));
    s->adp_census_ran = true;
    return 0;
}

int aqc_get_adapter_census(aqc_ctx* c, int which, int64_t out[1 + AQC_ADP_MAX_PROBES]) {
    if (!c || !out || !census_which(which)) return fail(AQC_ERR_ARG, "aqc_get_adapter_census: null argument or `which` is no pre-filter file");
    int rc = sync_all(c);
    if (rc) return rc;
    for (int k = 0; k < CEN_COUNTS; ++k) out[k] = 0;
    if (c->adp_census[which].acc) HIP_TRY(hipMemcpy(out, c->adp_census[which].acc, sizeof(int64_t) * CEN_COUNTS, hipMemcpyDeviceToHost));
    return 0;
}

// device time of the slot's last aqc_adapter_census; 0: it launched nothing
int aqc_adapter_census_ms(aqc_ctx* c, int slot, float* ms) {
    GET_SLOT(s);
    if (!ms) return fail(AQC_ERR_ARG, "aqc_adapter_census_ms: null argument");
    *ms = 0.f;
    if (!s->adp_census_ran) return 0;
    HIP_TRY(slot_sync(*s));
    HIP_TRY(hipEventElapsedTime(ms, s->adp_census_ev[0], s->adp_census_ev[1]));
    return 0;
}

}  // extern "C"
