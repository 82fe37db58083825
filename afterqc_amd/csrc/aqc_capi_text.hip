// aqc_capi_text.hip — the C API's text stages: FASTQ text framed on the device (aqc_frame, aqc_frame_mixed, aqc_reframe), the
// records formatted into their output streams (aqc_format and its variants, the fetchers of text, streams and span events), and
// the polyX census of a framed chunk (it stays with text in: aqc_census.hpp builds on aqc_textin.hpp).  The context, its slots
// and the shared helpers: aqc_ctx.hpp.
//
// Kernels launched here, and nowhere else (this is the one unit that includes these four headers):
//   aqc_textin.hpp    text_index_kernel, frame_records_kernel, frame_finish_kernel, parse_names_kernel
//   aqc_fmt.hpp       fmt_tile_sums_kernel, fmt_tile_bases_kernel
//   aqc_fmtcopy.hpp   fmt_plan_kernel, fmt_place_copy_kernel, fmt_plan_listed_kernel, fmt_copy_whole_kernel,
//                     fmt_copy_whole_list_kernel, fmt_copy_kernel
//   aqc_census.hpp    poly_census_kernel, census_names_kernel
// aqc_fast_args.hpp is here for FastWaveLds<>::PPW, the batch size of a fused placement (the verdict kernel's host-visible part: no
// device code).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <algorithm>

#include "aqc_ctx.hpp"
#include "aqc_prim.hpp"
#include "aqc_fast_args.hpp"
#include "aqc_textin.hpp"
#include "aqc_fmt.hpp"
#include "aqc_fmtcopy.hpp"
#include "aqc_census.hpp"

using namespace aqc;

extern "C" {

// t_scratch, one per slot: what the framing kernels and the formatter's sizing pass leave for each other and for the host.  aqc_frame
// and aqc_format take turns on the slot's stream, so the FrameOut and the stream totals share their place.
struct TextScratch {
    alignas(64) FrameMeta meta[2];
    alignas(64) unsigned long long lines[2];       // '\n' per file (text_index_kernel)
    union alignas(64) { FrameOut frame; unsigned long long fmt_totals[FMT_STREAMS]; };
};
constexpr size_t TEXT_SCRATCH_BYTES = 256;
static_assert(offsetof(TextScratch, lines) == 64 && offsetof(TextScratch, frame) == 128 && offsetof(TextScratch, fmt_totals) == 128 &&
              sizeof(TextScratch) <= TEXT_SCRATCH_BYTES, "the kernels of both stages were measured with these places");

// ---- text in -----------------------------------------------------------------------------------------------------
struct FrameExtents { const aqc_text_extent* ext[2]; uint64_t n[2]; uint8_t last[2]; };
// one aqc_frame call as its steps see the chunk
struct FrameJob {
    const aqc_text_chunk* ch;
    int nf;                        // files of the chunk: 2 when paired
    const uint8_t* text[2];
    uint64_t bytes[2];
    uint8_t* tbase[2];             // where each file's text begins on the device
    uint64_t tiles[2], cap[2];     // index tiles per file; entries its line table can take
    uint32_t virt[2];              // the line end that stands in for the '\n' an unterminated last line lacks (0: none)
    bool bubble;
};
constexpr size_t TEXT_SLACK = IDX_TILE + 64;

// parts of the chunk are in this device's memory already (aqc_frame_mixed): those move inside HBM, the rest comes up
static int put_extents(Slot* s, const FrameJob& j, int k, const FrameExtents& fx) {
    uint64_t cur = 0;
    for (uint64_t e = 0; e < fx.n[k]; ++e) {
        const aqc_text_extent& x = fx.ext[k][e];
        if (x.offset < cur || x.offset + x.bytes > j.bytes[k] || !x.device_text) return fail(AQC_ERR_ARG, "aqc_frame_mixed: extents must be sorted, disjoint and inside the chunk");
        if (x.offset > cur) HIP_TRY(hipMemcpyAsync(j.tbase[k] + cur, j.text[k] + cur, x.offset - cur, hipMemcpyHostToDevice, s->stream));
        if (x.bytes) HIP_TRY(hipMemcpyAsync(j.tbase[k] + x.offset, x.device_text, x.bytes, hipMemcpyDeviceToDevice, s->stream));
        cur = x.offset + x.bytes;
    }
    if (j.bytes[k] > cur) HIP_TRY(hipMemcpyAsync(j.tbase[k] + cur, j.text[k] + cur, j.bytes[k] - cur, hipMemcpyHostToDevice, s->stream));
    return 0;
}

// 1. text to the device (`resident`: it is there already, aqc_reframe).  The text sits TEXT_FRONT bytes into its buffer: the writer's
//    16-byte windows may start a few bytes before a piece's source.
static int put_text(Slot* s, FrameJob& j, int k, bool resident, const FrameExtents* fx) {
    Mate& m = s->m[k];
    if (m.seq.reserve(TEXT_FRONT + j.bytes[k] + TEXT_SLACK)) return fail(AQC_ERR_HIP, "hipMalloc of %llu bytes failed", (unsigned long long)j.bytes[k]);
    j.tbase[k] = (uint8_t*)m.seq.p + TEXT_FRONT;
    if (resident) return 0;
    const bool mixed = fx && fx->n[k];
    if (mixed) {
        const int rc = put_extents(s, j, k, *fx);
        if (rc) return rc;
    } else if (j.bytes[k]) HIP_TRY(hipMemcpyAsync(j.tbase[k], j.text[k], j.bytes[k], hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(j.tbase[k] + j.bytes[k], 0, TEXT_SLACK, s->stream));
    m.last_byte = !j.bytes[k] ? (uint8_t)'\n' : mixed ? fx->last[k] : j.text[k][j.bytes[k] - 1];
    return 0;
}

// 2. the file's share of the index launch and its line table
static int size_line_table(Slot* s, FrameJob& j, int k) {
    DevBuf& le = s->m[k].line_end;
    j.tiles[k] = j.bytes[k] ? (j.bytes[k] + IDX_TILE - 1) / IDX_TILE : 1;
    // FASTQ lines average ~90 bytes; a chunk with more lines than this guess is indexed again with the exact size
    const uint64_t guess = j.bytes[k] / 16 + 4096;
    j.cap[k] = le.cap / sizeof(uint32_t) > guess + 2 ? le.cap / sizeof(uint32_t) - 2 : guess;
    if (le.reserve(sizeof(uint32_t) * (j.cap[k] + 2))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    return 0;
}

// 3a. one attempt's launches: line index in one pass (text_index_kernel), both files in one launch; the four lines of every complete
//     group, the lock-step record count, the bytes consumed: all queued behind the index pass without asking the host for anything —
//     the kernels read the line totals where the index pass left them, their grids are sized for the most lines the chunk could hold
static int launch_index_and_frame(Slot* s, const FrameJob& j, TextScratch* sc) {
    const uint64_t all_tiles = j.tiles[0] + j.tiles[1];
    HIP_TRY(hipMemsetAsync(s->t_tile.p, 0, sizeof(unsigned long long) * (all_tiles + 1), s->stream));
    IndexFile f[2] = {};
    uint32_t t0 = 0;
    for (int k = 0; k < j.nf; k++) {
        f[k] = IndexFile{(const uint8_t*)j.tbase[k], j.bytes[k], (uint32_t*)s->m[k].line_end.p, j.cap[k], sc->lines + k, t0, (uint32_t)j.tiles[k]};
        t0 += (uint32_t)j.tiles[k];
    }
    hipLaunchKernelGGL(text_index_kernel, dim3((unsigned)all_tiles), dim3(TXT_BLOCK), 0, s->stream, f[0], f[1],
                       (unsigned long long*)s->t_tile.p, (unsigned int*)((unsigned long long*)s->t_tile.p + all_tiles));
    HIP_TRY(hipGetLastError());
    const FrameMeta init{0xffffffffu, 0u, 0xffffffffu, 0u};
    const FrameMeta h_meta[2] = {init, init};
    HIP_TRY(hipMemcpyAsync(sc->meta, h_meta, sizeof(h_meta), hipMemcpyHostToDevice, s->stream));
    uint64_t rec_cap = 0;
    for (int k = 0; k < j.nf; k++) {
        Mate& m = s->m[k];
        const uint64_t r = (j.cap[k] + 1) / 4 + 1;            // records the line table could describe
        rec_cap = std::max(rec_cap, r);
        if (m.off.reserve(4 * r) || m.qoff.reserve(4 * r) || m.len.reserve(4 * r) || m.name_off.reserve(4 * r) || m.name_len.reserve(4 * r) ||
            m.plus_off.reserve(4 * r) || m.plus_len.reserve(4 * r) || m.qual_len.reserve(4 * r))
            return fail(AQC_ERR_HIP, "hipMalloc failed");
        FramedFile ff{(uint32_t*)m.off.p, (uint32_t*)m.qoff.p, (uint32_t*)m.len.p, (uint32_t*)m.name_off.p,
                      (uint32_t*)m.name_len.p, (uint32_t*)m.plus_off.p, (uint32_t*)m.plus_len.p, (uint32_t*)m.qual_len.p};
        hipLaunchKernelGGL(frame_records_kernel, dim3((unsigned)((r + TXT_BLOCK - 1) / TXT_BLOCK)), dim3(TXT_BLOCK), 0, s->stream,
                           (const uint8_t*)j.tbase[k], (const uint32_t*)m.line_end.p, (const unsigned long long*)(sc->lines + k), j.virt[k], ff, sc->meta + k, (uint64_t)j.cap[k]);
    }
    // (a single-end chunk: line table 0 twice, see set_mate)
    hipLaunchKernelGGL(frame_finish_kernel, dim3(1), dim3(1), 0, s->stream, (const unsigned long long*)sc->lines, (const FrameMeta*)sc->meta,
                       (const uint32_t*)s->m[0].line_end.p, (const uint32_t*)s->m[j.nf - 1].line_end.p, (const uint32_t*)s->m[0].len.p,
                       j.virt[0], j.virt[1], (unsigned long long)j.bytes[0], (unsigned long long)j.bytes[1], j.nf, (unsigned long long)j.ch->max_records, &sc->frame,
                       (unsigned long long)j.cap[0], (unsigned long long)j.cap[1]);
    if (j.bubble) {
        // lane / tile / x / y out of the R1 names (preprocesser.py:180-192) for the bubble filter
        for (int k = 0; k < 5; k++)
            if (s->aux[k].reserve((k < 4 ? sizeof(int32_t) : 1) * rec_cap)) return fail(AQC_ERR_HIP, "hipMalloc failed");
        hipLaunchKernelGGL(parse_names_kernel, dim3((unsigned)((rec_cap + TXT_BLOCK - 1) / TXT_BLOCK)), dim3(TXT_BLOCK), 0, s->stream,
                           (const uint8_t*)j.tbase[0], (const uint32_t*)s->m[0].name_off.p, (const uint32_t*)s->m[0].name_len.p, (const unsigned long long*)&sc->frame.n,
                           (int32_t*)s->aux[0].p, (int32_t*)s->aux[1].p, (int32_t*)s->aux[2].p, (int32_t*)s->aux[3].p,
                           (uint8_t*)s->aux[4].p);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// 3b. index and frame: ONE copy back (FrameOut), ONE wait per chunk — and all of it once more for a chunk with more lines than its
//     table was sized for (counted, not written)
static int index_and_frame(Slot* s, FrameJob& j, FrameOut& fo) {
    TextScratch* sc = (TextScratch*)s->t_scratch.p;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int rc = launch_index_and_frame(s, j, sc);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(&fo, &sc->frame, sizeof(fo), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(slot_sync(*s));
        bool fits = true;
        for (int k = 0; k < j.nf; k++) {
            const uint64_t real = fo.lines[k] - (j.virt[k] ? 1 : 0);
            if (real > j.cap[k]) {
                fits = false;
                j.cap[k] = real;
                if (s->m[k].line_end.reserve(sizeof(uint32_t) * (j.cap[k] + 2))) return fail(AQC_ERR_HIP, "hipMalloc failed");
            }
        }
        if (fits) break;
    }
    return 0;
}

// 4. slot view: the text IS the arena, every kernel reads the records in place
// (a record whose quality line is not as long as its sequence line is a record like any other: fastq.py:37-49 does not look,
//  and every later stage keeps a view per string — LEN_IRR in aqc_batch.hpp)
static int publish_view(Slot* s, const FrameJob& j, const FrameOut& fo) {
    const uint64_t n = fo.n;
    DevBatch v{};
    v.n = n;
    v.first_index = j.ch->first_index;
    if (s->results.reserve(sizeof(aqc_result) * (n ? n : 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    // the quality lines' own lengths (frame_records_kernel) and room for the final quality views of the marked records
    // (written by the verdict kernels for those records only: no traffic for a regular chunk)
    s->has_irregular = fo.first_mismatch[0] < n || (j.nf == 2 && fo.first_mismatch[1] < n);
    for (int k = 0; k < j.nf; k++) {
        Mate& m = s->m[k];
        if (s->has_irregular && m.qview.reserve(sizeof(uint32_t) * (n ? n : 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
        set_mate(v, k, MateView{j.tbase[k], j.tbase[k], (const uint32_t*)m.off.p, (const uint32_t*)m.qoff.p, (const uint32_t*)m.len.p,
                                (const uint32_t*)m.qual_len.p, (uint32_t*)m.qview.p});
    }
    for (int k = 0; k < 2; k++) s->m[k].consumed = fo.consumed[k];      // (0 for the file a single-end chunk does not have)
    if (j.bubble) {
        v.aux_lane = (const int32_t*)s->aux[0].p; v.aux_tile = (const int32_t*)s->aux[1].p;
        v.aux_x = (const int32_t*)s->aux[2].p; v.aux_y = (const int32_t*)s->aux[3].p; v.aux_ok = (const uint8_t*)s->aux[4].p;
    }
    s->view = v;
    s->n = n;
    s->paired = j.nf == 2;
    s->raw_max_len = s->max_len = fo.max_len;
    return 0;
}

// 5. what the caller learns: the lock-step record count (preprocesser.py:412-429), the bytes consumed by the n records (+ R1's next
//    sequence length for the TOTAL_BASES quirk)
static void fill_frame_info(aqc_frame_info* info, const FrameOut& fo, bool paired) {
    memset(info, 0, sizeof(*info));
    info->n = fo.n;
    info->avail1 = fo.avail[0];
    info->avail2 = fo.avail[1];
    info->eof1 = (int32_t)fo.eof[0];
    info->eof2 = paired ? (int32_t)fo.eof[1] : 0;
    info->max_len = fo.max_len;
    info->consumed1 = fo.consumed[0];
    info->consumed2 = fo.consumed[1];
    info->next_len1 = fo.next_len1;
}

static int frame_impl(aqc_ctx* c, int slot, const aqc_text_chunk* ch, aqc_frame_info* info, bool resident, const FrameExtents* fx = nullptr) {
    GET_SLOT(s);
    if (!ch || !info || !ch->text1) return fail(AQC_ERR_ARG, "aqc_frame: null argument");
    const bool paired = ch->text2 != nullptr;
    FrameJob j{ch, paired ? 2 : 1, {ch->text1, ch->text2}, {ch->bytes1, paired ? ch->bytes2 : 0}};
    for (int k = 0; k < j.nf; k++)
        if (j.bytes[k] >= (1ull << 31) - IDX_TILE) return fail(AQC_ERR_ARG, "aqc_frame: chunks must be < 2 GiB");
    HIP_TRY(slot_sync(*s));
    s->framed = s->formatted = false;
    s->ran = false;
    s->fused = false;
    if (s->t_scratch.reserve(TEXT_SCRATCH_BYTES)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    int rc;
    for (int k = 0; k < j.nf; k++)
        if ((rc = put_text(s, j, k, resident, fx)) || (rc = size_line_table(s, j, k))) return rc;
    if (s->t_tile.reserve(sizeof(unsigned long long) * (j.tiles[0] + j.tiles[1] + 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    const int final_[2] = {ch->final1, ch->final2};
    for (int k = 0; k < j.nf; k++)      // an unterminated last line of the file is a line (readline() returns it); it may end in blanks
        if (final_[k] && j.bytes[k] > 0 && s->m[k].last_byte != '\n') j.virt[k] = (uint32_t)j.bytes[k] | LINE_WS;
    j.bubble = c->has_cfg && c->cfg.debubble;
    FrameOut fo{};
    if ((rc = index_and_frame(s, j, fo)) || (rc = publish_view(s, j, fo))) return rc;
    fill_frame_info(info, fo, paired);
    s->framed = true;
    s->last_chunk = *ch;
    return 0;
}

int aqc_frame(aqc_ctx* c, int slot, const aqc_text_chunk* ch, aqc_frame_info* info) { return frame_impl(c, slot, ch, info, false); }

int aqc_frame_mixed(aqc_ctx* c, int slot, const aqc_text_chunk* ch, const aqc_text_extent* ext1, uint64_t n_ext1, uint8_t last1,
                    const aqc_text_extent* ext2, uint64_t n_ext2, uint8_t last2, aqc_frame_info* info) {
    if ((n_ext1 && !ext1) || (n_ext2 && !ext2)) return fail(AQC_ERR_ARG, "aqc_frame_mixed: null extent list");
    const FrameExtents fx{{ext1, ext2}, {n_ext1, ch && ch->text2 ? n_ext2 : 0}, {last1, last2}};
    return frame_impl(c, slot, ch, info, false, &fx);
}

int aqc_reframe(aqc_ctx* c, int slot, aqc_frame_info* info) {
    GET_SLOT(s);
    if (!s->framed) return fail(AQC_ERR_STATE, "aqc_reframe needs a slot filled by aqc_frame");
    const aqc_text_chunk ch = s->last_chunk;
    return frame_impl(c, slot, &ch, info, true);
}

// ---- text out ----------------------------------------------------------------------------------------------------
static FormatView make_format_view(const aqc_ctx* c, const Slot* s, const Slot* vs, bool plain, int32_t store_overlap, bool spans) {
    FormatView v{};
    v.paired = s->paired ? 1 : 0;
    v.results = (const aqc_result*)vs->results.p;
    v.plain = plain ? 1 : 0;
    v.verdict_paired = vs->paired ? 1 : 0;
    v.barcode = c->cfg.barcode ? 1 : 0;
    v.barcode_length = c->cfg.barcode_length;
    // the third stream's mode: off, the merged reads of --store_merged, or (any other value) the overlap tails
    v.store_overlap = !(store_overlap && vs->paired) ? 0 : store_overlap == AQC_STORE_MERGED ? AQC_STORE_MERGED : AQC_STORE_OVERLAP;
    v.spans = (spans && !plain) ? 1 : 0;
    v.n_framed = s->n;
    v.consumed[0] = (uint32_t)s->m[0].consumed; v.consumed[1] = (uint32_t)s->m[1].consumed;
    for (int k = 0; k < (s->paired ? 2 : 1); k++) {
        const Mate& m = s->m[k];
        v.f[k].text = (const uint8_t*)m.seq.p + TEXT_FRONT;
        v.f[k].seq_off = (const uint32_t*)m.off.p;
        v.f[k].qual_off = (const uint32_t*)m.qoff.p;
        v.f[k].seq_len = (const uint32_t*)m.len.p;
        v.f[k].name_off = (const uint32_t*)m.name_off.p;
        v.f[k].name_len = (const uint32_t*)m.name_len.p;
        v.f[k].plus_off = (const uint32_t*)m.plus_off.p;
        v.f[k].plus_len = (const uint32_t*)m.plus_len.p;
        v.f[k].qual_len = (const uint32_t*)m.qual_len.p;
        v.f[k].qview = (const uint32_t*)m.qview.p;
    }
    return v;
}

// Stream sizes, the first way.  The verdict kernel may have done the placement already (AQC_FUSED=1, all n records of the slot, the
// two-stream case): its totals stand in for the sums / bases passes — unless it gave the placement up (a deferred pair, a record that
// is not plain text).  Taken: v.fused is set.
static int sizes_from_fused(Slot* s, FormatView& v, unsigned long long h_tot[FMT_STREAMS]) {
    unsigned long long misc[5];
    HIP_TRY(hipMemcpyAsync(misc, s->fz_misc.p, sizeof(misc), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if ((misc[0] >> 32) != 0) return 0;
    v.fused = 1;
    v.fstate[0] = (const uint32_t*)s->m[0].fz_rec.p; v.fstate[1] = (const uint32_t*)s->m[1].fz_rec.p;
    v.fbatch = (const unsigned long long*)s->fz_state.p;
    v.fbatch_shift = 5;
    static_assert(FastWaveLds<10, true, true>::PPW == 32, "fbatch_shift");
    h_tot[0] = misc[1]; h_tot[3] = misc[2]; h_tot[1] = misc[3]; h_tot[4] = misc[4];
    return 0;
}

// Stream sizes, the second way.  Streams q = file * 3 + {0 good, 1 bad, 2 overlap}: per-tile byte sums -> tile bases (one launch each),
// the per-record offsets are formed inside the writer.
// f_tile: [FMT_STREAMS x n_tiles] the tiles' prefixes inside their super-tiles | [FMT_STREAMS x n_super] the super-tiles' sums -> bases
static int sizes_from_sums(Slot* s, const FormatView& v, uint64_t n, uint64_t n_tiles, uint64_t n_super, unsigned long long h_tot[FMT_STREAMS]) {
    if (s->f_tile.reserve(sizeof(unsigned long long) * FMT_STREAMS * (n_tiles + n_super)) || s->t_scratch.reserve(TEXT_SCRATCH_BYTES))
        return fail(AQC_ERR_HIP, "hipMalloc failed");
    unsigned long long* d_tot = ((TextScratch*)s->t_scratch.p)->fmt_totals;
    unsigned long long* d_super = (unsigned long long*)s->f_tile.p + FMT_STREAMS * n_tiles;
    if (n) hipLaunchKernelGGL(fmt_tile_sums_kernel, dim3((unsigned)n_super), dim3(TXT_BLOCK), 0, s->stream, v, n, n_tiles, n_super, (unsigned long long*)s->f_tile.p, d_super);
    else HIP_TRY(hipMemsetAsync(s->f_tile.p, 0, sizeof(unsigned long long) * FMT_STREAMS * (n_tiles + n_super), s->stream));
    hipLaunchKernelGGL(fmt_tile_bases_kernel, dim3(v.spans ? FMT_STREAMS : 6), dim3(TXT_BLOCK), 0, s->stream, d_super, n_super, d_tot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot, d_tot, sizeof(unsigned long long) * (v.spans ? FMT_STREAMS : 6), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

// The writers' working buffers, carved once per call:
//   f_plan   one 16-byte plan word per (record, file), dense (`plan0`) | the six words of the records the general kernel takes, in list order (`listed`)
//   f_patch  the patch words of the dense plans | the one-piece plans of a spans / fused format, two words each, in list order (`wplan`)
//   f_pos    the general kernel's GEN_LISTS lists (`lists`) | their lengths (`n_gen`) | the lengths of the one-piece lists (`n_whole`)
//   f_over   full piece lists for the records that do not fit a plan
struct FormatLayout {
    uint64_t n_tasks, gen_cap, per_list;
    uint4 *plan0, *listed, *patch0, *wplan;
    FmtTask* over;
    uint32_t* lists;
    unsigned int *n_gen, *n_whole;
    unsigned list_blocks, copy_blocks;
};
static int carve_format_buffers(Slot* s, uint64_t n, uint64_t n_tiles, FormatLayout& L) {
    const int nf = s->paired ? 2 : 1;
    L.n_tasks = n * nf;
    L.gen_cap = ((n_tiles + GEN_LISTS - 1) / GEN_LISTS) * FMT_TILE * nf;     // worst case: every record
    const uint64_t plan0_bytes = (16 * L.n_tasks + 255) / 256 * 256;
    if (s->f_plan.reserve(plan0_bytes + 16 * PLAN_Q * L.gen_cap * GEN_LISTS) || s->f_patch.reserve(16 * L.n_tasks + 32 * L.gen_cap * GEN_LISTS) || s->f_over.reserve(sizeof(FmtTask) * L.n_tasks) ||
        s->f_pos.reserve(4 * L.gen_cap * GEN_LISTS + 2 * sizeof(unsigned int) * GEN_LISTS + 64))
        return fail(AQC_ERR_HIP, "hipMalloc failed");
    L.plan0 = (uint4*)s->f_plan.p;
    L.listed = (uint4*)((uint8_t*)s->f_plan.p + plan0_bytes);
    L.patch0 = (uint4*)s->f_patch.p;
    L.wplan = (uint4*)((uint8_t*)s->f_patch.p + 16 * L.n_tasks);
    L.over = (FmtTask*)s->f_over.p;
    L.lists = (uint32_t*)s->f_pos.p;
    L.n_gen = (unsigned int*)((uint8_t*)s->f_pos.p + 4 * L.gen_cap * GEN_LISTS);
    L.n_whole = L.n_gen + GEN_LISTS;
    // GEN_LISTS x k workgroups; k from the worst case, at most 32 per list
    L.per_list = std::min<uint64_t>(std::max<uint64_t>((L.gen_cap + GEN_ROUND - 1) / GEN_ROUND, 1), 32);
    L.list_blocks = (unsigned)(GEN_LISTS * L.per_list);
    L.copy_blocks = (unsigned)((L.n_tasks + (COPY_BLOCK / 32) * FMT_UNROLL - 1) / ((COPY_BLOCK / 32) * FMT_UNROLL));
    return 0;
}

// Which kernels write a pass (pass 1: the overlap streams of store_overlap).  The general copy kernel follows every one of them.
enum class Writer {
    PLACE_COPY,     // place + copy in one kernel, piece lists only for the listed records
    PLAN_WHOLE,     // dense plans, then the whole-record copy walks them
    PLAN_ONLY,      // dense-plan kernel alone: nothing for the whole-record copy to walk
    PLAN_LISTED,    // listed one-piece plans, then the list copy
};
static Writer choose_writer(const FormatView& v, int pass) {
    // text mode without barcodes, main pass (round 6): place + copy
    // (AQC_PLACE_COPY=0: the plan / whole-copy pair of rounds 2 - 5, for A/B measurements)
    static const bool place_copy = [] { const char* e = getenv("AQC_PLACE_COPY"); return !(e && e[0] == '0'); }();
    // spans / fused mode: what stays in the caller's chunk / what the verdict kernel copied has no plan; the records that are their
    // own bytes but for the walk's byte patches are still the plan kernel's, on a list
    const bool sparse = v.spans || v.fused;
    if (sparse) return Writer::PLAN_LISTED;
    if (place_copy && pass == 0 && !v.plain && !v.barcode) return Writer::PLACE_COPY;
    // a barcode run has no one-piece record: fmt_plan_kernel writes no dense plans and nothing walks them
    return v.barcode && !v.plain ? Writer::PLAN_ONLY : Writer::PLAN_WHOLE;
}

static void write_pass(Slot* s, const FormatView& v, const FormatLayout& L, const FormatOut& outs, int pass, uint64_t n, uint64_t n_tiles, uint64_t n_super) {
    const unsigned long long* tb = (const unsigned long long*)s->f_tile.p;
    const Writer w = choose_writer(v, pass);
    if (w == Writer::PLACE_COPY) {
        hipLaunchKernelGGL(fmt_place_copy_kernel, dim3((unsigned)n_tiles), dim3(PC_BLOCK), 0, s->stream, v, n, n_tiles, n_super, tb, tb + FMT_STREAMS * n_tiles,
                           L.listed, L.lists, L.n_gen, L.gen_cap, outs);
        hipLaunchKernelGGL(fmt_plan_listed_kernel, dim3(L.list_blocks), dim3(FMT_TILE), 0, s->stream, v, L.listed, L.over,
                           (const uint32_t*)L.lists, (const unsigned int*)L.n_gen, L.gen_cap, s->status);
    } else {
        hipLaunchKernelGGL(fmt_plan_kernel, dim3((unsigned)n_tiles), dim3(FMT_TILE), 0, s->stream, v, n, n_tiles, n_super,
                           tb, tb + FMT_STREAMS * n_tiles, pass, s->status, L.plan0, L.patch0,
                           L.listed, L.over, L.lists, L.n_gen, L.gen_cap, L.wplan, L.n_whole, outs.p[0], outs.p[3],
                           (SpanEvent*)s->m[0].f_events.p, (SpanEvent*)s->m[1].f_events.p);
        if (w == Writer::PLAN_WHOLE) hipLaunchKernelGGL(fmt_copy_whole_kernel, dim3(L.copy_blocks), dim3(COPY_BLOCK), 0, s->stream, v, L.n_tasks, (const uint4*)L.plan0,
                                                        (const uint4*)L.patch0, outs);
        if (w == Writer::PLAN_LISTED) hipLaunchKernelGGL(fmt_copy_whole_list_kernel, dim3(L.list_blocks), dim3(COPY_BLOCK), 0, s->stream, v, (const uint4*)L.wplan, outs,
                                                         (const unsigned int*)L.n_whole, L.gen_cap);
    }
    hipLaunchKernelGGL(fmt_copy_kernel, dim3(L.list_blocks), dim3(COPY_BLOCK), 0, s->stream, v,
                       (const uint4*)L.listed, (const FmtTask*)L.over, outs, (const uint32_t*)L.lists,
                       (const unsigned int*)L.n_gen, L.gen_cap);
}

static int format_impl(aqc_ctx* c, int slot, int verdict_slot, uint64_t n, int32_t store_overlap, uint64_t bytes_out[6], bool spans = false) {
    GET_SLOT(s);
    int rc;
    const bool plain = verdict_slot != slot;
    Slot* vs = s;
    if (plain && (rc = get_slot(c, verdict_slot, &vs))) return rc;
    if (!bytes_out) return fail(AQC_ERR_ARG, "aqc_format: null argument");
    if (!s->framed) return fail(AQC_ERR_STATE, "aqc_format needs a slot filled by aqc_frame");
    if (!vs->ran) return fail(AQC_ERR_STATE, "aqc_format before aqc_run");
    if (n > s->n || n > vs->n) return fail(AQC_ERR_ARG, "aqc_format: n exceeds the slot's records");
    if (plain) HIP_TRY(slot_sync(*vs));      // the verdicts come from another slot's stream
    FormatView v = make_format_view(c, s, vs, plain, store_overlap, spans);
    s->m[0].n_events = s->m[1].n_events = 0;
    const uint64_t n_tiles = n ? (n + FMT_TILE - 1) / FMT_TILE : 1;
    const uint64_t n_super = (n_tiles + FMT_SUPER - 1) / FMT_SUPER;
    unsigned long long h_tot[FMT_STREAMS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (s->fused && !plain && !spans && !v.store_overlap && n == s->n && n > 0 && (rc = sizes_from_fused(s, v, h_tot))) return rc;
    if (!v.fused) {
        s->fused = false;          // (whatever this call writes into the good streams replaces what the verdict kernel left there)
        if ((rc = sizes_from_sums(s, v, n, n_tiles, n_super, h_tot))) return rc;
    }
    for (int f = 0; f < (v.spans ? (s->paired ? 2 : 1) : 0); ++f) {
        s->m[f].n_events = h_tot[FMT_EVENT_STREAM + f];
        if (s->m[f].f_events.reserve(sizeof(SpanEvent) * (s->m[f].n_events + 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    }
    FormatOut outs{};
    for (int q = 0; q < 6; q++) {
        const bool live = (q < 3 || s->paired) && (q % 3 != 2 || v.store_overlap);
        s->f_bytes[q] = live ? h_tot[q] : 0;
        bytes_out[q] = s->f_bytes[q];
        if (s->f_out[q].reserve(s->f_bytes[q] + 64)) return fail(AQC_ERR_HIP, "hipMalloc failed");
        outs.p[q] = (uint8_t*)s->f_out[q].p;
    }
    if (n) {
        FormatLayout L;
        if ((rc = carve_format_buffers(s, n, n_tiles, L))) return rc;
        for (int pass = 0; pass < (v.store_overlap ? 2 : 1); ++pass) {
            if (pass == 1 && v.store_overlap == AQC_STORE_MERGED) {
                // the merged reads: a kernel of its own, file 0's third stream (index records have none)
                if (!plain) {
                    const unsigned long long* tb = (const unsigned long long*)s->f_tile.p;
                    hipLaunchKernelGGL(fmt_merged_kernel, dim3((unsigned)n_tiles), dim3(FMT_TILE), 0, s->stream, v, n, n_tiles, n_super, tb, tb + FMT_STREAMS * n_tiles,
                                       s->status, outs.p[2]);
                }
                continue;
            }
            HIP_TRY(hipMemsetAsync(L.n_gen, 0, 2 * sizeof(unsigned int) * GEN_LISTS, s->stream));
            write_pass(s, v, L, outs, pass, n, n_tiles, n_super);
        }
        HIP_TRY(hipGetLastError());
    }
    s->formatted = true;
    s->formatted_fused = v.fused != 0;
    s->compressed = false;
    return 0;
}

int aqc_format(aqc_ctx* c, int slot, uint64_t n, int32_t store_overlap, uint64_t bytes_out[6]) {
    return format_impl(c, slot, slot, n, store_overlap, bytes_out);
}

int aqc_format_spans(aqc_ctx* c, int slot, uint64_t n, int32_t store_overlap, uint64_t bytes_out[6], uint64_t n_events[2]) {
    if (!n_events) return fail(AQC_ERR_ARG, "aqc_format_spans: null argument");
    const int rc = format_impl(c, slot, slot, n, store_overlap, bytes_out, true);
    if (rc) return rc;
    n_events[0] = c->slots[slot].m[0].n_events;
    n_events[1] = c->slots[slot].m[1].n_events;
    return 0;
}

int aqc_format_fused(aqc_ctx* c, int slot) {
    GET_SLOT(s);
    if (!s->formatted) return fail(AQC_ERR_STATE, "aqc_format_fused before aqc_format");
    return s->formatted_fused ? 1 : 0;
}

int aqc_span_end(aqc_ctx* c, int slot, uint64_t n, uint64_t end[2]) {
    GET_SLOT(s);
    if (!s->framed || !end || n > s->n) return fail(AQC_ERR_ARG, "aqc_span_end: bad arguments");
    for (int f = 0; f < 2; ++f) {
        end[f] = 0;
        if (f == 1 && !s->paired) break;
        if (n == s->n) { end[f] = s->m[f].consumed; continue; }
        uint32_t off = 0;               // record n begins where record n - 1 ends
        HIP_TRY(hipMemcpyAsync(&off, (const uint32_t*)s->m[f].name_off.p + n, sizeof(off), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        end[f] = off;
    }
    return 0;
}

int aqc_format_plain(aqc_ctx* c, int slot, int verdict_slot, uint64_t n, int32_t store_overlap, uint64_t bytes_out[6]) {
    if (slot == verdict_slot) return fail(AQC_ERR_ARG, "aqc_format_plain: the verdicts must come from another slot");
    return format_impl(c, slot, verdict_slot, n, store_overlap, bytes_out);
}

int aqc_fetch_text(aqc_ctx* c, int slot, int file, int stream, uint8_t* dst, uint64_t cap) {
    GET_SLOT(s);
    if (!s->formatted) return fail(AQC_ERR_STATE, "aqc_fetch_text before aqc_format");
    if (file < 0 || file > 1 || stream < 0 || stream > 2) return fail(AQC_ERR_ARG, "aqc_fetch_text: bad file/stream");
    const int q = file * 3 + stream;
    return fetch_out(*s, s->f_out[q].p, s->f_bytes[q], dst, cap, "aqc_fetch_text");
}

int aqc_fetch_streams(aqc_ctx* c, int slot, int32_t gz, uint8_t* const dst[6], const uint64_t cap[6]) {
    GET_SLOT(s);
    if (!dst || !cap) return fail(AQC_ERR_ARG, "aqc_fetch_streams: null argument");
    if (!s->formatted) return fail(AQC_ERR_STATE, "aqc_fetch_streams before aqc_format");
    if (gz && !s->compressed) return fail(AQC_ERR_STATE, "aqc_fetch_streams(gz) before aqc_compress");
    for (int q = 0; q < 6; ++q) {
        const uint64_t nb = gz ? s->g_bytes[q] : s->f_bytes[q];
        if (!nb) continue;
        if (!dst[q] || nb > cap[q]) return fail(AQC_ERR_ARG, "aqc_fetch_streams: stream %d (%llu bytes) does not fit", q, (unsigned long long)nb);
        HIP_TRY(hipMemcpyAsync(dst[q], gz ? s->g_packed[q].p : s->f_out[q].p, nb, hipMemcpyDeviceToHost, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return check_status(*s);
}

int aqc_fetch_span_events(aqc_ctx* c, int slot, int file, aqc_span_event* dst, uint64_t cap) {
    GET_SLOT(s);
    if (!s->formatted) return fail(AQC_ERR_STATE, "aqc_fetch_span_events before aqc_format_spans");
    if (file < 0 || file > 1) return fail(AQC_ERR_ARG, "aqc_fetch_span_events: bad file");
    static_assert(sizeof(aqc_span_event) == sizeof(SpanEvent), "host and device event layouts must agree");
    const uint64_t ne = s->m[file].n_events;
    // (this entry counts in events, not bytes, and says so)
    if (ne > cap) return fail(AQC_ERR_ARG, "aqc_fetch_span_events: %llu events do not fit %llu", (unsigned long long)ne, (unsigned long long)cap);
    return fetch_out(*s, s->m[file].f_events.p, sizeof(SpanEvent) * ne, dst, sizeof(SpanEvent) * ne, "aqc_fetch_span_events");
}

// ---- debubble pre-pass: polyX census (aqc_census.hpp) ------------------------------------------------------------
int aqc_poly_census(aqc_ctx* c, int slot, int32_t poly_max, uint64_t* n_hits) {
    GET_SLOT(s);
    int rc;
    if (!n_hits || poly_max < 1) return fail(AQC_ERR_ARG, "aqc_poly_census: null argument or poly_max < 1");
    if (!s->framed) return fail(AQC_ERR_STATE, "aqc_poly_census needs a slot filled by aqc_frame");
    if (s->paired) return fail(AQC_ERR_ARG, "aqc_poly_census: the census reads single-end slots (one file per chunk)");
    *n_hits = 0;
    s->n_census = 0;
    const uint64_t n = s->n;
    if (s->census_hits.reserve(sizeof(aqc_census_hit) * (n ? n : 1)) || s->census_n.reserve(sizeof(unsigned long long)))
        return fail(AQC_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemsetAsync(s->census_n.p, 0, sizeof(unsigned long long), s->stream));
    if (n) {
        const DevBatch& v = s->view;
        for (hipEvent_t& e : s->census_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(s->census_ev[0], s->stream));
        const uint64_t per_block = (uint64_t)TXT_BLOCK * CENSUS_PER_THREAD;
        hipLaunchKernelGGL(poly_census_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(TXT_BLOCK), 0, s->stream, v.seq1, v.off1,
                           v.len1, (const uint32_t*)s->m[0].name_off.p, (const uint32_t*)s->m[0].name_len.p, n, (int)poly_max, v.first_index,
                           (aqc_census_hit*)s->census_hits.p, (unsigned long long*)s->census_n.p, s->status);
        // (grid-strided over the hits, whose number only the device knows here: at most 4 workgroups per CU)
        const uint64_t name_blocks = std::min<uint64_t>((n + TXT_BLOCK - 1) / TXT_BLOCK, (uint64_t)c->n_cu * 4);
        hipLaunchKernelGGL(census_names_kernel, dim3((unsigned)name_blocks), dim3(TXT_BLOCK), 0, s->stream, v.seq1,
                           (aqc_census_hit*)s->census_hits.p, (const unsigned long long*)s->census_n.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(s->census_ev[1], s->stream));
    }
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, s->census_n.p, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    rc = check_status(*s);
    if (rc) return rc;
    s->n_census = h;
    *n_hits = h;
    return 0;
}

int aqc_census_ms(aqc_ctx* c, int slot, float* ms) {
    GET_SLOT(s);
    if (!ms) return fail(AQC_ERR_ARG, "aqc_census_ms: null argument");
    *ms = 0.f;
    if (s->census_ev[1]) HIP_TRY(hipEventElapsedTime(ms, s->census_ev[0], s->census_ev[1]));
    return 0;
}

int aqc_fetch_census(aqc_ctx* c, int slot, aqc_census_hit* dst, uint64_t cap) {
    GET_SLOT(s);
    if (!dst && cap) return fail(AQC_ERR_ARG, "aqc_fetch_census: null destination");
    const uint64_t m = std::min(cap, s->n_census);
    if (m) {
        HIP_TRY(hipMemcpyAsync(dst, s->census_hits.p, sizeof(aqc_census_hit) * m, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return 0;
}

}  // extern "C"
