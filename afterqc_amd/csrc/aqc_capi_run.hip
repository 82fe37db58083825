// aqc_capi_run.hip — the C API's verdict stage: a batch up to the device (aqc_upload), the verdict kernels (aqc_run), the results
// back (aqc_fetch_results, aqc_fetch_quality_views, aqc_last_deferred, aqc_last_verdict_words), the three function seams and the libed.so pair; and the
// .gz output stage (aqc_compress, aqc_fetch_gz).  The context, its slots and the shared helpers: aqc_ctx.hpp.
//
// Why .gz out is here and not in a unit of its own: gz_encode_kernel does not compile to the same instructions there.  In a unit
// without the verdict kernels the compiler leaves the bit writer's flush loop (GzSinkEmit::flush_words) rolled; beside them, as
// in the single unit this API used to be, it peels it.  Nothing in the source ties the two, so the encoder stays with the
// verdict kernels until it can be measured on its own (profiles/r11_capi_split.txt).
//
// Kernels launched here, and nowhere else (this is the one unit that includes aqc_upload.hpp, aqc_record.hpp, aqc_seams.hpp and
// aqc_gzdev.hpp + aqc_gzlz.hpp; the member, bit-ring and symbol functions the three encoders share are in aqc_gzdev.hpp and
// aqc_deflate_sym.hpp):
//   aqc_upload.hpp   narrow_offsets_kernel, mark_irregular_kernel, quality_views_kernel
//   aqc_record.hpp   filter_overlap_kernel, filter_overlap_list_kernel, filter_overlap_cut_kernel<LIST>
//   aqc_fast.hpp     fast_filter_overlap_kernel<NW, PAIRED, WPBT, BARCODE, FUSE, CUT> (a template: the variants are instantiated here)
//   aqc_viewpass.hpp no kernel of its own: the frame of the three view passes in front of the verdict kernel, and their dispatch on G
//   aqc_qcut.hpp     quality_cut_kernel<G> (the quality cut's pass, and its function seam)
//   aqc_adapter.hpp  adapter_cut_kernel<G> (the adapter pass behind it, a second producer of the same views, and its function seam)
//   aqc_polytail.hpp poly_tail_kernel<G> (the poly-G / poly-X pass behind both, a third producer, and its function seam)
//   aqc_gzdev.hpp    gz_hist_kernel, gz_encode_wave_kernel, gz_encode_kernel, gz_offsets_kernel, gz_pack_kernel
//   aqc_gzlz.hpp     gz_hist_lz_kernel, gz_encode_lz_kernel (levels 6 - 9)
//   aqc_seams.hpp    overlap_seam_kernel, read_stats_seam_kernel, edit_distance_seam_kernel, edit_distance_any_kernel,
//                    seek_overlap_kernel
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <vector>

#include "aqc_ctx.hpp"
#include "aqc_prim.hpp"
#include "aqc_upload.hpp"
#include "aqc_record.hpp"
#include "aqc_seams.hpp"
#include "aqc_fast.hpp"
#include "aqc_gzdev.hpp"
#include "aqc_gzlz.hpp"
#include "aqc_gz.hpp"
#include <zlib.h>

using namespace aqc;

// a pass in front of the verdict kernel leaves a view per mate and record: the quality cut, the adapter pass, the poly-tail pass, or several
static bool views_on(const aqc_ctx* c) { return qcut_on(c->cut) || adp_on(c->adapter) || poly_on(c->poly); }

constexpr int FUSE_WPBT = 12;      // waves per workgroup of the fused verdict kernel
// waves per workgroup of the 20-word tier's paired instances: 10 or 11 fit the CU's 160 KiB of LDS (144,048 / 157,568 bytes).  11 by
// measurement: 3 - 4 % faster than 10 at 2 x 300 and 2 x 317, interleaved builds (profiles/r14_tier20.txt); -DAQC_TIER20_WPBT=10
// builds the other one to repeat it
#ifndef AQC_TIER20_WPBT
#define AQC_TIER20_WPBT 11
#endif
constexpr int TIER20_WPBT_PAIRED = AQC_TIER20_WPBT;
static_assert(TIER20_WPBT_PAIRED == 10 || TIER20_WPBT_PAIRED == 11, "the 20-word rows of 10 or 11 waves fit a CU's LDS");
template <int NW, bool PAIRED, int WPBT, bool BARCODE, bool FUSE = false, bool CUT = false>
static void launch_fast(aqc_ctx* c, Slot* s, const aqc_config& cfg, const DevStats& st, uint64_t accum_limit, const FuseArgs* fz = nullptr) {
    constexpr uint64_t per_block = (uint64_t)WPBT * FastWaveLds<NW, PAIRED, FUSE>::PPW;
    uint64_t blocks = (s->n + per_block - 1) / per_block;
    // persistent grid: as many workgroups as the LDS footprint lets a CU hold; batches are grid-strided
    const size_t lds = sizeof(FastWaveLds<NW, PAIRED, FUSE>) * WPBT + sizeof(BlockAcc) + 64 + 17 * 16 + (FUSE ? 16 * 8 : 0);
    uint64_t per_cu = (160 * 1024) / lds;
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    const uint64_t cap = (uint64_t)c->n_cu * per_cu;
    if (blocks > cap) blocks = cap;
    // pairs the fast kernel cannot decide exactly (exotic bytes, very short reads, ...) are queued and
    // finished by the general wave-per-record pipeline right behind it on the same stream
    (void)hipMemsetAsync(s->n_deferred.p, 0, sizeof(unsigned int), s->stream);
    FastArgs K;
    K.fb = s->view; K.cfg = cfg; K.circ = c->circles; K.results = (aqc_result*)s->results.p; K.st = st; K.accum_limit = accum_limit;
    K.deferred = (uint32_t*)s->deferred.p; K.n_deferred = (unsigned int*)s->n_deferred.p;
    K.fz = fz ? *fz : FuseArgs{};
    if constexpr (CUT) {
        // (the cut's instances take the view array — the mates of a record side by side — behind the arguments every instance takes)
        FastCutArgs KC;
        static_cast<FastArgs&>(KC) = K;
        KC.cut = (const uint32_t*)s->cut.p;
        hipLaunchKernelGGL((fast_filter_overlap_kernel<NW, PAIRED, WPBT, false, false, true>), dim3((unsigned)blocks), dim3(WPBT * WAVE), 0, s->stream, KC);
    } else
        hipLaunchKernelGGL((fast_filter_overlap_kernel<NW, PAIRED, WPBT, BARCODE, FUSE>), dim3((unsigned)blocks), dim3(WPBT * WAVE), 0, s->stream, K);
}

// one tier of the lane-per-pair kernel (NW words per read; waves per workgroup for pairs / single reads): paired x barcode
template <int NW, int WPBT_PAIRED, int WPBT_SINGLE>
static void launch_fast_tier(aqc_ctx* c, Slot* s, const aqc_config& cfg, const DevStats& st, uint64_t accum_limit) {
    if (views_on(c)) {      // (never with a barcode: aqc_run refuses that)
        if (cfg.paired) launch_fast<NW, true, WPBT_PAIRED, false, false, true>(c, s, cfg, st, accum_limit);
        else launch_fast<NW, false, WPBT_SINGLE, false, false, true>(c, s, cfg, st, accum_limit);
        return;
    }
    if (cfg.paired) { if (cfg.barcode) launch_fast<NW, true, WPBT_PAIRED, true>(c, s, cfg, st, accum_limit); else launch_fast<NW, true, WPBT_PAIRED, false>(c, s, cfg, st, accum_limit); }
    else { if (cfg.barcode) launch_fast<NW, false, WPBT_SINGLE, true>(c, s, cfg, st, accum_limit); else launch_fast<NW, false, WPBT_SINGLE, false>(c, s, cfg, st, accum_limit); }
}

// (`front` readable bytes before the data as well: read 2 is loaded in 16-byte chunks counted from its END, the chunk
// with a read's first bases may begin up to 16 bytes before the read)
static int up(DevBuf& d, const void* src, size_t bytes, hipStream_t st, size_t front = 0) {
    if (d.reserve(front + bytes + ARENA_SLACK)) return fail(AQC_ERR_HIP, "hipMalloc of %zu bytes failed", bytes);
    if (bytes == 0) return 0;
    HIP_TRY(hipMemcpyAsync((uint8_t*)d.p + front, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
}

// 64-bit host offsets -> 32-bit device offsets (through the slot's staging buffer, in stream order)
static int up_offsets(Slot& s, DevBuf& d, const uint64_t* src, uint64_t n) {
    if (d.reserve(sizeof(uint32_t) * (n ? n : 1)) || s.off_stage.reserve(sizeof(uint64_t) * (n ? n : 1)))
        return fail(AQC_ERR_HIP, "hipMalloc failed");
    if (n == 0) return 0;
    HIP_TRY(hipMemcpyAsync(s.off_stage.p, src, sizeof(uint64_t) * n, hipMemcpyHostToDevice, s.stream));
    hipLaunchKernelGGL(narrow_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, (const uint64_t*)s.off_stage.p,
                       (uint32_t*)d.p, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One mate of a batch up to the device, in this order on the stream: arena, quality arena, 32-bit offsets, quality offsets, lengths.
// What is left in `mv` is the mate as the kernels see it.  `qual == seq` (one arena holds both strings): the view aliases, nothing more
// goes up.  The caller says how long the quality arena is, and how many readable bytes the arena needs in front (see up()).
struct MateSrc { const uint8_t *seq, *qual; const uint64_t *off, *qoff; const uint32_t* len; uint64_t bytes, qbytes; };
static int upload_mate(Slot& s, int k, const MateSrc& b, uint64_t n, bool need_qual, size_t front, MateView& mv) {
    Mate& m = s.m[k];
    int rc;
    if ((rc = up(m.seq, b.seq, b.bytes, s.stream, front))) return rc;
    mv.seq = (const uint8_t*)m.seq.p + front;
    if (b.qual && need_qual) {
        if (b.qual == b.seq) mv.qual = mv.seq;
        else {
            if ((rc = up(m.qual, b.qual, b.qbytes, s.stream))) return rc;
            mv.qual = (const uint8_t*)m.qual.p;
        }
    } else if (need_qual) return fail(AQC_ERR_ARG, "batch: qual%d is required", k + 1);
    if ((rc = up_offsets(s, m.off, b.off, n))) return rc;
    mv.off = (const uint32_t*)m.off.p;
    if (b.qoff) {
        if ((rc = up_offsets(s, m.qoff, b.qoff, n))) return rc;
        mv.qoff = (const uint32_t*)m.qoff.p;
    }
    if ((rc = up(m.len, b.len, sizeof(uint32_t) * n, s.stream))) return rc;
    mv.len = (const uint32_t*)m.len.p;
    return 0;
}

// quality strings with lengths of their own: the mates that differ are marked in the device copy of their length words
static int upload_quality_lengths(Slot& s, const aqc_batch* b, uint64_t n, int nm, MateView mv[2]) {
    if (nm == 2 && !b->qlen2) return fail(AQC_ERR_ARG, "batch: qlen1 without qlen2");
    const uint32_t* ql[2] = {b->qlen1, b->qlen2};
    for (int k = 0; k < nm; ++k) {
        Mate& m = s.m[k];
        const int rc = up(m.qlen, ql[k], sizeof(uint32_t) * n, s.stream);
        if (rc) return rc;
        if (m.qview.reserve(sizeof(uint32_t) * (n ? n : 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
        if (n) hipLaunchKernelGGL(mark_irregular_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, (uint32_t*)m.len.p,
                                  (const uint32_t*)m.qlen.p, n);
        mv[k].qlen = (const uint32_t*)m.qlen.p;
        mv[k].qview = (uint32_t*)m.qview.p;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

static int fill_slot(aqc_ctx* c, Slot& s, const aqc_batch* b, bool need_qual, bool need_pair) {
    const uint64_t n = b->n;
    if (!b->seq1 || !b->off1 || !b->len1) return fail(AQC_ERR_ARG, "batch: seq1/off1/len1 are required");
    const bool paired = b->seq2 != nullptr;
    if (need_pair && !paired) return fail(AQC_ERR_ARG, "batch: this call needs seq2/off2/len2");
    if (paired && (!b->off2 || !b->len2)) return fail(AQC_ERR_ARG, "batch: off2/len2 missing");
    if (n >= (1ull << 31)) return fail(AQC_ERR_ARG, "batch: more than 2^31 records (split the batch)");
    const uint64_t lim = (1ull << 32) - 4096;      // 32-bit byte offsets on the device, chunk loads may run 320 bytes (16 x the widest tier's 20 words) past a read's start
    if (b->bytes1 >= lim || b->qbytes1 >= lim || b->bytes2 >= lim || b->qbytes2 >= lim) return fail(AQC_ERR_ARG, "batch: an arena must be smaller than 4 GiB (split the batch)");
    // make sure earlier work on this slot has drained before its buffers are overwritten / regrown
    HIP_TRY(slot_sync(s));
    int rc;
    const int nm = paired ? 2 : 1;
    MateView mv[2] = {};
    // a quality arena without a size of its own is as long as the sequences'; read 2 alone gets TEXT_FRONT bytes in front of its arena
    if ((rc = upload_mate(s, 0, MateSrc{b->seq1, b->qual1, b->off1, b->qoff1, b->len1, b->bytes1, b->qbytes1 ? b->qbytes1 : b->bytes1}, n, need_qual, 0, mv[0]))) return rc;
    if (paired && (rc = upload_mate(s, 1, MateSrc{b->seq2, b->qual2, b->off2, b->qoff2, b->len2, b->bytes2, b->qbytes2 ? b->qbytes2 : b->bytes2}, n, need_qual, TEXT_FRONT, mv[1]))) return rc;
    DevBatch v{};
    v.n = n;
    v.first_index = b->first_index;
    if (b->aux_ok && b->aux_lane && b->aux_tile && b->aux_x && b->aux_y) {
        const void* src[5] = {b->aux_lane, b->aux_tile, b->aux_x, b->aux_y, b->aux_ok};
        for (int k = 0; k < 5; k++)
            if ((rc = up(s.aux[k], src[k], (k < 4 ? sizeof(int32_t) : 1) * n, s.stream))) return rc;
        v.aux_lane = (const int32_t*)s.aux[0].p;
        v.aux_tile = (const int32_t*)s.aux[1].p;
        v.aux_x = (const int32_t*)s.aux[2].p;
        v.aux_y = (const int32_t*)s.aux[3].p;
        v.aux_ok = (const uint8_t*)s.aux[4].p;
    }
    if (s.results.reserve(sizeof(aqc_result) * (n ? n : 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    s.has_irregular = b->qlen1 != nullptr && need_qual;
    if (s.has_irregular && (rc = upload_quality_lengths(s, b, n, nm, mv))) return rc;
    for (int k = 0; k < nm; ++k) set_mate(v, k, mv[k]);
    uint32_t mx = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (b->len1[i] > mx) mx = b->len1[i];
        if (paired && b->len2[i] > mx) mx = b->len2[i];
    }
    s.raw_max_len = mx;
    s.view = v;
    s.n = n;
    s.paired = paired;
    s.ran = false;
    return 0;
}

// ---- the view passes.  What a launch of any of them is given: the mates' fixed trims, one view per mate and record into `view`
// (n_mates per record), the four counts into `stats` (may be NULL), and — the passes behind the quality cut — the views the mates
// come with (view_in: may be `view`; NULL: everything)
struct ViewPassJob {
    int32_t trim_front[2], trim_tail[2];
    int n_mates;
    const uint32_t* view_in;
    uint32_t* view;
    unsigned long long* stats;
    uint64_t accum_limit;
};

// the pass's kernel over the slot's records: kernel_of(G) names its instance for G lanes per read
template <class Args, class KernelOf>
static int launch_pass(aqc_ctx* c, Slot& s, const Args& A, KernelOf kernel_of) {
    vp_dispatch(view_pass_lanes(s), s.n, c->n_cu, [&](auto G, dim3 grid, dim3 block) { hipLaunchKernelGGL(kernel_of(G), grid, block, 0, s.stream, A); });
    HIP_TRY(hipGetLastError());
    return 0;
}

// the quality cut's pass (aqc_qcut.hpp): it reads the quality lines through the batch view, and no views come in
static int launch_cut(aqc_ctx* c, Slot& s, const QcutOpts& o, const ViewPassJob& j) {
    QcutArgs A{};
    A.b = s.view; A.o = o; A.n_mates = j.n_mates; A.view = j.view; A.stats = j.stats; A.accum_limit = j.accum_limit; A.status = s.status;
    for (int k = 0; k < 2; ++k) { A.trim_front[k] = j.trim_front[k]; A.trim_tail[k] = j.trim_tail[k]; }
    return launch_pass(c, s, A, [](auto G) { return quality_cut_kernel<decltype(G)::value>; });
}

// the sequence-line passes (aqc_adapter.hpp, aqc_polytail.hpp): mate k's lines in the slot's batch view and its fixed trim ...
static ViewMate view_mate(const Slot& s, const ViewPassJob& j, int k) {
    return ViewMate{k ? s.view.seq2 : s.view.seq1, k ? s.view.off2 : s.view.off1, k ? s.view.len2 : s.view.len1, j.trim_front[k], j.trim_tail[k]};
}
// ... and the frame fields their *Args share
template <class Args>
static void fill_frame(Args& A, const Slot& s, const ViewPassJob& j) {
    A.n = s.view.n; A.n_mates = j.n_mates; A.view_in = j.view_in; A.view = j.view; A.stats = j.stats; A.accum_limit = j.accum_limit; A.status = s.status;
}

static int launch_adapter(aqc_ctx* c, Slot& s, const AdapterOpts& a, const ViewPassJob& j) {
    AdapterArgs A{};
    fill_frame(A, s, j);
    A.min_overlap = a.min_overlap;
    for (int k = 0; k < j.n_mates; ++k) {
        A.m[k].v = view_mate(s, j, k);
        A.m[k].alen = a.len[k];
        for (int i = 0; i < ADP_WORDS; ++i) A.m[k].w[i] = a.w[k][i];
    }
    return launch_pass(c, s, A, [](auto G) { return adapter_cut_kernel<decltype(G)::value>; });
}

static int launch_poly(aqc_ctx* c, Slot& s, const PolyOpts& o, const ViewPassJob& j) {
    PolyArgs A{};
    fill_frame(A, s, j);
    for (int x = 0; x < POLY_LETTERS; ++x) A.min_len[x] = o.min_len[x];
    for (int k = 0; k < j.n_mates; ++k) A.m[k] = view_mate(s, j, k);
    return launch_pass(c, s, A, [](auto G) { return poly_tail_kernel<decltype(G)::value>; });
}

extern "C" {

// ---- upload and run ----------------------------------------------------------------------------------------------
int aqc_upload(aqc_ctx* c, int slot, const aqc_batch* b) {
    GET_SLOT(s);
    int rc;
    if (!b) return fail(AQC_ERR_ARG, "null batch");
    if ((rc = fill_slot(c, *s, b, true, false))) return rc;
    s->framed = s->formatted = false;
    s->max_len = s->raw_max_len;
    return 0;
}

static int grid_for(const aqc_ctx* c, uint64_t n) {
    // persistent grid: enough workgroups to fill every CU several times over, records grid-strided
    uint64_t blocks = (n + WPB - 1) / WPB;
    uint64_t cap = (uint64_t)c->n_cu * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

// What aqc_run launches for the slot's records: the general wave-per-record kernel, or the lane-per-pair kernel whenever its
// preconditions hold: one of its four tiers by the longest read, or its fused instance.
enum class Verdict { GENERAL, TIER10, TIER16, TIER18, TIER20, FUSED };
// words per read of the lane-per-pair instance (aqc_last_verdict_words); 0: the general kernel
static int verdict_words(Verdict k) { return k == Verdict::GENERAL ? 0 : k == Verdict::TIER16 ? 16 : k == Verdict::TIER18 ? 18 : k == Verdict::TIER20 ? 20 : 10; }
static Verdict choose_verdict_kernel(const aqc_ctx* c, const Slot& s, const aqc_config& cfg) {
    const int thr = cfg.qualified_quality_phred + 33;
    // barcodes on that kernel: detectBarcode's three windows must lie in the first 32 bases and the verify sequence must
    // be plain A/C/G/T (2-bit codes); anything else takes the general kernel
    bool barcode_ok = true;
    if (cfg.barcode) {
        barcode_ok = cfg.barcode_verify_len >= 1 && cfg.barcode_length + 1 + cfg.barcode_verify_len <= 31;
        for (int j = 0; j < cfg.barcode_verify_len && barcode_ok; ++j) {
            const uint8_t ch = cfg.barcode_verify[j];
            barcode_ok = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
        }
    }
    if (c->force_generic || !barcode_ok || thr < 0 || thr > 127 || s.max_len > 320 || s.max_len == 0) return Verdict::GENERAL;
    // AQC_FUSED=1: pairs of device-framed text whose records are plain four-line text are placed in their output
    // streams by the verdict kernel itself, which also copies the good records that go out as their own bytes
    // (31-bit stream offsets; a bad record grows by its flag text)
    // (not with the quality cut or an adapter on: their instances are the plain tiers)
    if (c->fuse_opt && !views_on(c) && s.framed && cfg.paired && !cfg.barcode && s.max_len <= 160 && !s.has_irregular && s.m[0].consumed + 16 * s.n < (1ull << 31) &&
        s.m[1].consumed + 16 * s.n < (1ull << 31))
        return Verdict::FUSED;
    // (TIER18, 257 .. 288 bases: 2x250 reads that still carry a barcode + verify prefix (BASELINE config 5: 267 bases))
    // (TIER20, 289 .. 320 bases: the 2x300 kit, written as 300 or 301 cycles, with or without that prefix (317 bases))
    return s.max_len <= 160 ? Verdict::TIER10 : s.max_len <= 256 ? Verdict::TIER16 : s.max_len <= 288 ? Verdict::TIER18 : Verdict::TIER20;
}

// the fused placement's buffers: look-back words per batch, position words per record, ticket | abort | totals, the two good streams
static int prepare_fuse(Slot& s, FuseArgs& fz) {
    constexpr uint64_t PPW = FastWaveLds<10, true, true>::PPW;
    const uint64_t n_batches = (s.n + PPW - 1) / PPW;
    if (s.fz_state.reserve(16 * n_batches) || s.m[0].fz_rec.reserve(4 * s.n) || s.m[1].fz_rec.reserve(4 * s.n) || s.fz_misc.reserve(64) ||
        s.f_out[0].reserve(s.m[0].consumed + 64) || s.f_out[3].reserve(s.m[1].consumed + 64))
        return fail(AQC_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemsetAsync(s.fz_state.p, 0, 16 * n_batches, s.stream));
    HIP_TRY(hipMemsetAsync(s.fz_misc.p, 0, 64, s.stream));
    fz.name_off1 = (const uint32_t*)s.m[0].name_off.p; fz.name_off2 = (const uint32_t*)s.m[1].name_off.p;
    fz.out1 = (uint8_t*)s.f_out[0].p; fz.out2 = (uint8_t*)s.f_out[3].p;
    fz.fstate1 = (uint32_t*)s.m[0].fz_rec.p; fz.fstate2 = (uint32_t*)s.m[1].fz_rec.p;
    fz.state = (unsigned long long*)s.fz_state.p;
    fz.ticket = (unsigned int*)s.fz_misc.p; fz.abort = (int*)s.fz_misc.p + 1; fz.totals = (unsigned long long*)s.fz_misc.p + 1;
    return 0;
}

// A view pass of an aqc_run: both mates' views into the slot's array, timed by an event pair of its own.  The first pass that runs
// fills the array; a pass behind it — the views come in if any pass with a smaller ViewPassId ran — updates them in place.
static int run_view_pass(aqc_ctx* c, Slot& s, ViewPassId which, const aqc_config& cfg, uint64_t accum_limit) {
    ViewPass& vp = s.pass[which];
    const int nm = cfg.paired ? 2 : 1;
    if (s.cut.reserve(sizeof(uint32_t) * s.n * nm)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    for (hipEvent_t& e : vp.ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    uint32_t* const view = (uint32_t*)s.cut.p;
    bool earlier = false;
    for (int p = 0; p < which; ++p) earlier = earlier || s.pass[p].ran;
    const ViewPassJob j{{cfg.trim_front, cfg.trim_front2}, {cfg.trim_tail, cfg.trim_tail2}, nm, earlier ? view : nullptr, view, c->pass_stats[which].p, accum_limit};
    HIP_TRY(hipEventRecord(vp.ev[0], s.stream));
    const int rc = which == VP_CUT ? launch_cut(c, s, c->cut, j) : which == VP_ADAPTER ? launch_adapter(c, s, c->adapter, j) : launch_poly(c, s, c->poly, j);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(vp.ev[1], s.stream));
    vp.ran = true;
    return 0;
}

int aqc_run(aqc_ctx* c, int slot, uint64_t accum_limit) {
    GET_SLOT(s);
    if (!c->has_cfg) return fail(AQC_ERR_STATE, "aqc_run before aqc_set_config");
    if (c->cfg.paired && !s->paired) return fail(AQC_ERR_STATE, "config says paired but the slot holds single-end records");
    if (c->cfg.debubble && c->circles.n > 0 && !s->view.aux_ok) return fail(AQC_ERR_ARG, "debubble needs the aux_* arrays");
    const bool cut = views_on(c);           // the verdict kernels take views: the CUT instances
    if (cut && c->cfg.barcode) return fail(AQC_ERR_UNSUPPORTED, "aqc_run: the quality cut, an adapter or a poly-tail cut together with a barcode is not implemented");
    s->fused = false;
    s->verdict_words = 0;
    for (ViewPass& vp : s->pass) vp.ran = false;
    if (s->n == 0) { s->ran = true; return 0; }
    aqc_config cfg = c->cfg;
    if (!cfg.paired) cfg.no_overlap = 1;
    DevStats st{c->counters, c->ovl_hist, c->dist_hist, s->status, err_key_of(*s)};
    s->err_record = UINT64_MAX;
    if (s->qc.pending()) HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_qc, 0));      // (statRead of the previous run still reads the results)
    const bool pass_on[VP_N] = {qcut_on(c->cut), adp_on(c->adapter), poly_on(c->poly)};
    for (int p = 0; p < VP_N; ++p)
        if (pass_on[p]) {
            const int rc = run_view_pass(c, *s, (ViewPassId)p, cfg, accum_limit);
            if (rc) return rc;
        }
    HIP_TRY(hipEventRecord(launch_event(*s, AQC_K_FILTER_OVERLAP, 0), s->stream));
    const Verdict k = choose_verdict_kernel(c, *s, cfg);
    s->used_fast = k != Verdict::GENERAL;
    s->verdict_words = verdict_words(k);
    // (with the cut on, the general kernel and the deferred list's take the views behind their usual arguments)
    FilterCutArgs fc{FilterArgs{s->view, cfg, c->circles, (aqc_result*)s->results.p, st, accum_limit}, nullptr, nullptr,
                     (const uint32_t*)s->cut.p};
    if (k == Verdict::GENERAL) {
        if (cut) hipLaunchKernelGGL(filter_overlap_cut_kernel<false>, dim3(grid_for(c, s->n)), dim3(BLOCK), 0, s->stream, fc);
        else hipLaunchKernelGGL(filter_overlap_kernel, dim3(grid_for(c, s->n)), dim3(BLOCK), 0, s->stream, s->view, cfg, c->circles,
                           (aqc_result*)s->results.p, st, accum_limit);
    } else {
        if (s->deferred.reserve(sizeof(uint32_t) * (s->n + 1)) || s->n_deferred.reserve(sizeof(unsigned int)))
            return fail(AQC_ERR_HIP, "hipMalloc failed");
        if (k == Verdict::FUSED) {
            FuseArgs fz{};
            const int rc = prepare_fuse(*s, fz);
            if (rc) return rc;
            launch_fast<10, true, FUSE_WPBT, false, true>(c, s, cfg, st, accum_limit, &fz);
            s->fused = true;
        } else if (k == Verdict::TIER10) launch_fast_tier<10, 16, 12>(c, s, cfg, st, accum_limit);
        else if (k == Verdict::TIER16) launch_fast_tier<16, 12, 11>(c, s, cfg, st, accum_limit);
        else if (k == Verdict::TIER18) launch_fast_tier<18, 12, 10>(c, s, cfg, st, accum_limit);
        else launch_fast_tier<20, TIER20_WPBT_PAIRED, 9>(c, s, cfg, st, accum_limit);
        fc.list = (const uint32_t*)s->deferred.p;
        fc.n_list = (const unsigned int*)s->n_deferred.p;
        if (cut) hipLaunchKernelGGL(filter_overlap_cut_kernel<true>, dim3((unsigned)c->n_cu), dim3(BLOCK), 0, s->stream, fc);
        else hipLaunchKernelGGL(filter_overlap_list_kernel, dim3((unsigned)c->n_cu), dim3(BLOCK), 0, s->stream, s->view, cfg, c->circles,
                           (aqc_result*)s->results.p, st, accum_limit, (const uint32_t*)s->deferred.p,
                           (const unsigned int*)s->n_deferred.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(launch_event(*s, AQC_K_FILTER_OVERLAP, 1), s->stream));
    s->timed[AQC_K_FILTER_OVERLAP] = !s->collecting;
    s->ran = true;
    return 0;
}

// ---- results -----------------------------------------------------------------------------------------------------
int aqc_fetch_results(aqc_ctx* c, int slot, aqc_result* out, uint64_t n) {
    GET_SLOT(s);
    if (!s->ran) return fail(AQC_ERR_STATE, "aqc_fetch_results before aqc_run");
    if (n > s->n) return fail(AQC_ERR_ARG, "aqc_fetch_results: n exceeds the slot's records");
    if (n) HIP_TRY(hipMemcpyAsync(out, s->results.p, sizeof(aqc_result) * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(slot_sync(*s));
    return check_status(*s);
}

int aqc_fetch_quality_views(aqc_ctx* c, int slot, int mate, uint32_t* out, uint64_t n) {
    GET_SLOT(s);
    if (!s->ran) return fail(AQC_ERR_STATE, "aqc_fetch_quality_views before aqc_run");
    if (n > s->n || !out || mate < 0 || mate > 1 || (mate == 1 && !s->paired)) return fail(AQC_ERR_ARG, "aqc_fetch_quality_views: bad arguments");
    if (n == 0) return 0;
    if (s->off_stage.reserve(sizeof(uint32_t) * n)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    hipLaunchKernelGGL(quality_views_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->view, (const aqc_result*)s->results.p, mate,
                       (uint32_t*)s->off_stage.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, s->off_stage.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(slot_sync(*s));
    return 0;
}

// the time of a view pass of the slot's last aqc_run; 0: it launched none
static int view_pass_ms(aqc_ctx* c, int slot, ViewPassId which, float* ms, const char* who) {
    GET_SLOT(s);
    if (!ms) return fail(AQC_ERR_ARG, "%s: null argument", who);
    *ms = 0.f;
    const ViewPass& vp = s->pass[which];
    if (!vp.ran) return 0;
    HIP_TRY(slot_sync(*s));
    HIP_TRY(hipEventElapsedTime(ms, vp.ev[0], vp.ev[1]));
    return 0;
}
int aqc_cut_ms(aqc_ctx* c, int slot, float* ms) { return view_pass_ms(c, slot, VP_CUT, ms, "aqc_cut_ms"); }
int aqc_adapter_ms(aqc_ctx* c, int slot, float* ms) { return view_pass_ms(c, slot, VP_ADAPTER, ms, "aqc_adapter_ms"); }
int aqc_poly_ms(aqc_ctx* c, int slot, float* ms) { return view_pass_ms(c, slot, VP_POLY, ms, "aqc_poly_ms"); }

// (host state only: set by aqc_run when it chose the kernel, so there is nothing to wait for)
int aqc_last_verdict_words(aqc_ctx* c, int slot) {
    GET_SLOT(s);
    if (!s->ran) return fail(AQC_ERR_STATE, "aqc_last_verdict_words before aqc_run");
    return s->verdict_words;
}

int aqc_last_deferred(aqc_ctx* c, int slot, uint32_t* idx, uint64_t cap, uint64_t* n) {
    GET_SLOT(s);
    if (!n) return fail(AQC_ERR_ARG, "aqc_last_deferred: null argument");
    if (!s->ran) return fail(AQC_ERR_STATE, "aqc_last_deferred before aqc_run");
    HIP_TRY(slot_sync(*s));
    *n = 0;
    if (!s->used_fast || !s->n_deferred.p) return 0;
    unsigned int m = 0;
    HIP_TRY(hipMemcpy(&m, s->n_deferred.p, sizeof(m), hipMemcpyDeviceToHost));
    *n = m;
    const uint64_t w = m < cap ? m : cap;
    if (idx && w) HIP_TRY(hipMemcpy(idx, s->deferred.p, sizeof(uint32_t) * w, hipMemcpyDeviceToHost));
    return 0;
}

// ---- gzip output on the device (aqc_gzdev.hpp) --------------------------------------------------------------------------------
static int ensure_gz_tables(aqc_ctx* c) {
    if (c->gz_crc.p) return 0;
    GzCrcTables t;
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t v = i;
        for (int k = 0; k < 8; ++k) v = (v >> 1) ^ (0xEDB88320u & (0u - (v & 1u)));
        t.byte_table[i] = v;
    }
    // "advance the CRC register by n zero bytes" is linear: column j is what zlib's crc32_combine makes of the unit vector
    for (int k = 0; k < 8; ++k)
        for (int j = 0; j < 32; ++j) t.shift[k][j] = (uint32_t)crc32_combine((uLong)(1u << j), 0UL, (z_off_t)(GZ_SEG << k));
    if (c->gz_crc.reserve(sizeof(t))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpy(c->gz_crc.p, &t, sizeof(t), hipMemcpyHostToDevice));
    return 0;
}

int aqc_compress(aqc_ctx* c, int slot, int32_t level, uint64_t gz_bytes_out[6]) {
    GET_SLOT(s);
    int rc;
    if (!gz_bytes_out) return fail(AQC_ERR_ARG, "aqc_compress: null argument");
    if (!s->formatted) return fail(AQC_ERR_STATE, "aqc_compress before aqc_format");
    if (level < 1) return fail(AQC_ERR_UNSUPPORTED, "aqc_compress: level %d (stored output is the host writer's business)", level);
    if (level > 9) return fail(AQC_ERR_ARG, "aqc_compress: level %d (1 .. 9)", level);
    if ((rc = ensure_gz_tables(c))) return rc;
    static_assert(sizeof(GzCodebookDev) == sizeof(aqcgz::GzCodebook), "host and device codebook layouts must agree");
    GzJob J{};
    uint32_t n_members = 0;
    // members of 64 x 255 bytes, a wave each (round 6: gz_encode_wave_kernel); AQC_GZ_ENCODER=seg: members of 256 x 255 bytes, a
    // thread per 255-byte segment (gz_encode_kernel, rounds 3 - 5)
    static const bool wave_enc = [] { const char* e = getenv("AQC_GZ_ENCODER"); return !(e && e[0] == 's'); }();
    // levels 6 - 9: members of 256 x 255 bytes with a hash-chain match search, a wave each (gz_encode_lz_kernel, aqc_gzlz.hpp);
    // AQC_GZ_LZ=0 sends them down the path of levels 1 - 5
    static const bool lz_on = [] { const char* e = getenv("AQC_GZ_LZ"); return !(e && e[0] == '0'); }();
    const bool lz = level >= 6 && lz_on;
    const bool wave_members = wave_enc && !lz;
    J.member_text = wave_members ? (uint32_t)GZW_TEXT : (uint32_t)GZ_TEXT;
    J.slot_bytes = wave_members ? (uint32_t)GZW_SLOT : (uint32_t)GZ_SLOT;
    for (int q = 0; q < 6; ++q) {
        J.text[q] = (const uint8_t*)s->f_out[q].p;
        J.bytes[q] = s->f_bytes[q];
        J.first_block[q] = n_members;
        n_members += (uint32_t)((s->f_bytes[q] + J.member_text - 1) / J.member_text);
        s->g_bytes[q] = 0;
        gz_bytes_out[q] = 0;
    }
    J.first_block[6] = n_members;
    // (`compressed` is set once the streams exist: an error on the way must not let aqc_fetch_gz hand out empty streams)
    if (n_members == 0) { s->compressed = true; return 0; }
    if (s->g_stage.reserve((size_t)n_members * J.slot_bytes) || s->g_sizes.reserve(4 * (size_t)n_members) || s->g_offsets.reserve(8 * (size_t)n_members) ||
        s->g_total.reserve(64) || s->g_hist.reserve(6 * 320 * 4) || s->g_code.reserve(6 * sizeof(GzCodebookDev)))
        return fail(AQC_ERR_HIP, "hipMalloc failed");
    for (int q = 0; q < 6; ++q) {
        const uint64_t nb = J.first_block[q + 1] - J.first_block[q];
        if (s->g_packed[q].reserve(nb * (J.member_text + 31) + 64)) return fail(AQC_ERR_HIP, "hipMalloc failed");
        J.packed[q] = (uint8_t*)s->g_packed[q].p;
    }
    J.stage = (uint8_t*)s->g_stage.p; J.sizes = (uint32_t*)s->g_sizes.p; J.offsets = (uint64_t*)s->g_offsets.p; J.total = (uint64_t*)s->g_total.p;
    J.hist = (uint32_t*)s->g_hist.p; J.code = (const GzCodebookDev*)s->g_code.p; J.crc = (const GzCrcTables*)c->gz_crc.p;
    // 1. symbol counts of a sample of every stream's members
    HIP_TRY(hipMemsetAsync(s->g_hist.p, 0, 6 * 320 * 4, s->stream));
    if (lz) hipLaunchKernelGGL(gz_hist_lz_kernel, dim3(6 * GZ_SAMPLES), dim3(WAVE), 0, s->stream, J, gzlz_depth(level));
    else hipLaunchKernelGGL(gz_hist_kernel, dim3(6 * GZ_SAMPLES), dim3(GZ_THREADS), 0, s->stream, J);
    HIP_TRY(hipGetLastError());
    uint32_t h[6][320];
    HIP_TRY(hipMemcpyAsync(h, s->g_hist.p, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    // 2. one code per stream, built on the host with the routines of its own encoder
    std::vector<aqcgz::GzCodebook> cb(6);
    for (int q = 0; q < 6; ++q)
        if (!aqcgz::build_codebook(h[q], h[q] + 286, &cb[q])) return fail(AQC_ERR_STATE, "aqc_compress: could not build a Huffman code");
    HIP_TRY(hipMemcpyAsync(s->g_code.p, cb.data(), 6 * sizeof(aqcgz::GzCodebook), hipMemcpyHostToDevice, s->stream));
    // 3. members, their places, the contiguous streams
    if (lz) hipLaunchKernelGGL(gz_encode_lz_kernel, dim3(n_members), dim3(WAVE), 0, s->stream, J, gzlz_depth(level));
    else if (wave_enc) hipLaunchKernelGGL(gz_encode_wave_kernel, dim3(n_members), dim3(WAVE), 0, s->stream, J);
    else hipLaunchKernelGGL(gz_encode_kernel, dim3(n_members), dim3(GZ_THREADS), 0, s->stream, J);
    hipLaunchKernelGGL(gz_offsets_kernel, dim3(6), dim3(GZ_THREADS), 0, s->stream, J);
    hipLaunchKernelGGL(gz_pack_kernel, dim3(n_members), dim3(GZ_THREADS), 0, s->stream, J);
    HIP_TRY(hipGetLastError());
    unsigned long long tot[6];
    HIP_TRY(hipMemcpyAsync(tot, s->g_total.p, sizeof(tot), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));      // (cb and tot live on this stack frame)
    for (int q = 0; q < 6; ++q) {
        s->g_bytes[q] = tot[q];
        gz_bytes_out[q] = tot[q];
    }
    rc = check_status(*s);
    s->compressed = rc == 0;
    return rc;
}

int aqc_fetch_gz(aqc_ctx* c, int slot, int file, int stream, uint8_t* dst, uint64_t cap) {
    GET_SLOT(s);
    if (!s->compressed) return fail(AQC_ERR_STATE, "aqc_fetch_gz before aqc_compress");
    if (file < 0 || file > 1 || stream < 0 || stream > 2) return fail(AQC_ERR_ARG, "aqc_fetch_gz: bad file/stream");
    const int q = file * 3 + stream;
    return fetch_out(*s, s->g_packed[q].p, s->g_bytes[q], dst, cap, "aqc_fetch_gz");
}

// ---- function seams: run on a scratch slot (the last one) -------------------------------------------
static int seam_prepare(aqc_ctx* c, const aqc_batch* b, bool need_qual, bool need_pair, Slot** out) {
    if (!c || !b) return fail(AQC_ERR_ARG, "null argument");
    Slot* s;
    int rc = get_slot(c, c->n_slots - 1, &s);
    if (rc) return rc;
    if ((rc = fill_slot(c, *s, b, need_qual, need_pair))) return rc;
    for (uint64_t i = 0; i < b->n; i++)
        if (b->len1[i] > AQC_MAX_READ_LEN || (need_pair && b->len2[i] > AQC_MAX_READ_LEN))
            return fail(AQC_ERR_READ_TOO_LONG, "record %llu is longer than %d", (unsigned long long)i, AQC_MAX_READ_LEN);
    *out = s;
    return 0;
}

static int seam_out_bytes(Slot* s, DevBuf& d, void* host, size_t bytes) {
    if (bytes) HIP_TRY(hipMemcpyAsync(host, d.p, bytes, hipMemcpyDeviceToHost, s->stream));
    return 0;
}
#define seam_out(s, d, host, n) seam_out_bytes(s, d, host, sizeof(*(host)) * (n))

int aqc_overlap(aqc_ctx* c, const aqc_batch* b, int32_t* offset, int32_t* overlap_len, int32_t* diff) {
    Slot* s;
    int rc = seam_prepare(c, b, false, true, &s);
    if (rc) return rc;
    const uint64_t n = b->n;
    if (n == 0) return 0;
    DevBuf o[3];
    for (auto& d : o)
        if (d.reserve(4 * n)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    hipLaunchKernelGGL(overlap_seam_kernel, dim3((unsigned)((n + WPB - 1) / WPB)), dim3(BLOCK), 0, s->stream, s->view,
                       (int32_t*)o[0].p, (int32_t*)o[1].p, (int32_t*)o[2].p);
    HIP_TRY(hipGetLastError());
    if ((rc = seam_out(s, o[0], offset, n)) || (rc = seam_out(s, o[1], overlap_len, n)) || (rc = seam_out(s, o[2], diff, n))) return rc;
    HIP_TRY(slot_sync(*s));
    return 0;
}

int aqc_read_stats(aqc_ctx* c, const aqc_batch* b, int32_t max_poly, int32_t mismatch, int32_t qual, uint8_t* polyx,
                   int32_t* low_qual, int32_t* n_count) {
    Slot* s;
    int rc = seam_prepare(c, b, true, false, &s);
    if (rc) return rc;
    const uint64_t n = b->n;
    if (n == 0) return 0;
    DevBuf o[3];
    if (o[0].reserve(n) || o[1].reserve(4 * n) || o[2].reserve(4 * n)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    hipLaunchKernelGGL(read_stats_seam_kernel, dim3((unsigned)((n + WPB - 1) / WPB)), dim3(BLOCK), 0, s->stream, s->view,
                       max_poly, mismatch, qual, (uint8_t*)o[0].p, (int32_t*)o[1].p, (int32_t*)o[2].p);
    HIP_TRY(hipGetLastError());
    if ((rc = seam_out(s, o[0], polyx, n)) || (rc = seam_out(s, o[1], low_qual, n)) || (rc = seam_out(s, o[2], n_count, n))) return rc;
    HIP_TRY(slot_sync(*s));
    return 0;
}

int aqc_edit_distance(aqc_ctx* c, const aqc_batch* b, int32_t* dist) {
    Slot* s;
    int rc = seam_prepare(c, b, false, true, &s);
    if (rc) return rc;
    const uint64_t n = b->n;
    if (n == 0) return 0;
    DevBuf o;
    if (o.reserve(4 * n)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    hipLaunchKernelGGL(edit_distance_seam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->view,
                       (int32_t*)o.p, s->status);
    HIP_TRY(hipGetLastError());
    if ((rc = seam_out(s, o, dist, n))) return rc;
    HIP_TRY(slot_sync(*s));
    return check_status(*s);
}

// The function seam of a view pass: read 1 of the batch through the pass alone, one view per record out.  view_in (may be NULL): the
// views the reads come with, uploaded into the array the pass then updates in place.  launch(slot, job) starts the kernel.
using SeamLaunch = std::function<int(Slot&, const ViewPassJob&)>;
static int view_seam(aqc_ctx* c, const aqc_batch* b, bool need_qual, int32_t trim_front, int32_t trim_tail, const uint32_t* view_in, uint32_t* view,
                     const SeamLaunch& launch) {
    Slot* s;
    int rc = seam_prepare(c, b, need_qual, false, &s);
    if (rc) return rc;
    const uint64_t n = b->n;
    if (n == 0) return 0;
    DevBuf out;
    if (out.reserve(4 * n)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    if (view_in) HIP_TRY(hipMemcpyAsync(out.p, view_in, 4 * n, hipMemcpyHostToDevice, s->stream));
    uint32_t* const v = (uint32_t*)out.p;
    if ((rc = launch(*s, ViewPassJob{{trim_front, 0}, {trim_tail, 0}, 1, view_in ? v : nullptr, v, nullptr, UINT64_MAX}))) return rc;
    if ((rc = seam_out(s, out, view, n))) return rc;
    HIP_TRY(slot_sync(*s));
    return check_status(*s);
}

int aqc_quality_cut_views(aqc_ctx* c, const aqc_batch* b, const aqc_cut_config* cut, int32_t trim_front, int32_t trim_tail, uint32_t* view) {
    if (!cut || !view) return fail(AQC_ERR_ARG, "aqc_quality_cut_views: null argument");
    const QcutOpts o{cut->front ? 1 : 0, cut->tail ? 1 : 0, cut->right ? 1 : 0, cut->window, cut->mean_quality};
    if (!qcut_opts_ok(o) || trim_front < 0 || trim_tail < 0) return fail(AQC_ERR_ARG, "aqc_quality_cut_views: window / mean quality / trim out of range");
    return view_seam(c, b, true, trim_front, trim_tail, nullptr, view, [&](Slot& s, const ViewPassJob& j) { return launch_cut(c, s, o, j); });
}

// ... of a sequence-line pass: `cfg` its options as the caller gave them, opts_ok: they are in range (`what`: their names in the error
// text).  The pass reads sequence lines only; a batch that brings quality lines is taken as aqc_run takes it, LEN_IRR marks included.
static int line_pass_seam(aqc_ctx* c, const aqc_batch* b, const char* who, const void* cfg, bool opts_ok, const char* what, int32_t trim_front,
                          int32_t trim_tail, const uint32_t* view_in, uint32_t* view, const SeamLaunch& launch) {
    if (!cfg || !view) return fail(AQC_ERR_ARG, "%s: null argument", who);
    if (!opts_ok || trim_front < 0 || trim_tail < 0) return fail(AQC_ERR_ARG, "%s: %s / trim out of range", who, what);
    return view_seam(c, b, b && b->qual1 != nullptr, trim_front, trim_tail, view_in, view, launch);
}

int aqc_adapter_views(aqc_ctx* c, const aqc_batch* b, const aqc_adapter_config* adapter, int32_t trim_front, int32_t trim_tail, const uint32_t* view_in,
                      uint32_t* view) {
    AdapterOpts a{};
    const bool ok = adp_from_config(adapter, a);
    return line_pass_seam(c, b, "aqc_adapter_views", adapter, ok, "adapter / min overlap", trim_front, trim_tail, view_in, view,
                          [&](Slot& s, const ViewPassJob& j) { return launch_adapter(c, s, a, j); });
}

int aqc_poly_views(aqc_ctx* c, const aqc_batch* b, const aqc_poly_config* poly, int32_t trim_front, int32_t trim_tail, const uint32_t* view_in,
                   uint32_t* view) {
    PolyOpts o{};
    const bool ok = poly_from_config(poly, o);
    return line_pass_seam(c, b, "aqc_poly_views", poly, ok, "minimum length", trim_front, trim_tail, view_in, view,
                          [&](Slot& s, const ViewPassJob& j) { return launch_poly(c, s, o, j); });
}

// ---- the reference's existing native seam: libed.so (editdistance/_editdistance.h:16,23, loaded by util.py:16-24) ----
// Same two symbols, same signatures, so that `cdll.LoadLibrary(<this library>)` serves util.editDistance (util.py:70) and
// util.overlap_hm_cpp (util.py:223).  Device-backed like everything else here (one lazily created context on GPU 0, one
// small launch per call); no error channel exists in these signatures, so a failure is printed and the "none" value
// of the interface comes back (0xFFFFFFFF / 0x7FFFFFFF).
static std::mutex g_compat_mu;
static aqc_ctx* g_compat = nullptr;
// (on the heap and never deleted: a static DevBuf would call hipFree from a static destructor at exit(), in no fixed order
//  against the HIP runtime's own tear-down)
static DevBuf* const g_compat_buf = new DevBuf[4];

static int compat_prepare(const char* a, size_t la, const char* b, size_t lb, size_t row_bytes) {
    if (!g_compat) {
        int rc = aqc_create(0, 1, &g_compat);
        if (rc) { g_compat = nullptr; return rc; }
    }
    HIP_TRY(hipSetDevice(g_compat->device));
    if (g_compat_buf[0].reserve(la + 16) || g_compat_buf[1].reserve(lb + 16) || g_compat_buf[2].reserve(row_bytes + 16) ||
        g_compat_buf[3].reserve(16))
        return fail(AQC_ERR_HIP, "hipMalloc failed");
    if (la) HIP_TRY(hipMemcpy(g_compat_buf[0].p, a, la, hipMemcpyHostToDevice));
    if (lb) HIP_TRY(hipMemcpy(g_compat_buf[1].p, b, lb, hipMemcpyHostToDevice));
    return 0;
}

unsigned int edit_distance(const char* a, const unsigned int asize, const char* b, const unsigned int bsize) {
    if (asize == 0) return bsize;                    // (_editdistance.cpp:101-102)
    if (bsize == 0) return asize;
    std::lock_guard<std::mutex> g(g_compat_mu);
    int out = -1;
    if (compat_prepare(a, asize, b, bsize, sizeof(int) * ((size_t)bsize + 1)) == 0) {
        hipLaunchKernelGGL(edit_distance_any_kernel, dim3(1), dim3(WAVE), 0, 0, (const uint8_t*)g_compat_buf[0].p, (int)asize,
                           (const uint8_t*)g_compat_buf[1].p, (int)bsize, (int*)g_compat_buf[2].p, (int*)g_compat_buf[3].p);
        if (hipMemcpy(&out, g_compat_buf[3].p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) out = -1;
    }
    if (out < 0) fprintf(stderr, "libafterqc_hip: edit_distance failed: %s\n", aqc_last_error());
    return (unsigned int)out;
}

int seek_overlap(const char* r1, const int len1, const char* r2, const int len2, const int limit_distance,
                 const int complete_compare_require, const int overlap_require) {
    std::lock_guard<std::mutex> g(g_compat_mu);
    int out = 0x7FFFFFFF;
    bool ok = len1 >= 0 && len2 >= 0 && compat_prepare(r1, (size_t)len1, r2, (size_t)len2, 0) == 0;
    if (ok) {
        hipLaunchKernelGGL(seek_overlap_kernel, dim3(1), dim3(WAVE), 0, 0, (const uint8_t*)g_compat_buf[0].p, len1,
                           (const uint8_t*)g_compat_buf[1].p, len2, limit_distance, complete_compare_require, overlap_require,
                           (int*)g_compat_buf[3].p);
        ok = hipMemcpy(&out, g_compat_buf[3].p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) { fprintf(stderr, "libafterqc_hip: seek_overlap failed: %s\n", aqc_last_error()); out = 0x7FFFFFFF; }
    return out;
}


}  // extern "C"
