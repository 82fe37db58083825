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
// aqc_fast.hpp is here for FastWaveLds<>::PPW, the batch size of a fused placement (it defines a template kernel only, and none
// of it is instantiated in this unit).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <algorithm>

#include "aqc_ctx.hpp"
#include "aqc_prim.hpp"
#include "aqc_fast.hpp"
#include "aqc_textin.hpp"
#include "aqc_fmt.hpp"
#include "aqc_fmtcopy.hpp"
#include "aqc_census.hpp"

using namespace aqc;

extern "C" {

// ---- text in -----------------------------------------------------------------------------------------------------
struct FrameExtents { const aqc_text_extent* ext[2]; uint64_t n[2]; uint8_t last[2]; };
static int frame_impl(aqc_ctx* c, int slot, const aqc_text_chunk* ch, aqc_frame_info* info, bool resident, const FrameExtents* fx = nullptr) {
    GET_SLOT(s);
    if (!ch || !info || !ch->text1) return fail(AQC_ERR_ARG, "aqc_frame: null argument");
    const bool paired = ch->text2 != nullptr;
    const int nf = paired ? 2 : 1;
    const uint8_t* text[2] = {ch->text1, ch->text2};
    const uint64_t bytes[2] = {ch->bytes1, paired ? ch->bytes2 : 0};
    const int final_[2] = {ch->final1, ch->final2};
    for (int k = 0; k < nf; k++)
        if (bytes[k] >= (1ull << 31) - IDX_TILE) return fail(AQC_ERR_ARG, "aqc_frame: chunks must be < 2 GiB");
    HIP_TRY(slot_sync(*s));
    s->framed = s->formatted = false;
    s->ran = false;
    s->fused = false;
    DevBuf* arena[2] = {&s->seq1, &s->seq2};
    DevBuf* seq_off[2] = {&s->off1, &s->off2};
    DevBuf* qual_off[2] = {&s->qoff1, &s->qoff2};
    DevBuf* seq_len[2] = {&s->len1, &s->len2};
    // scratch: FrameMeta[2] | line totals[2] | tail values[4]
    if (s->t_scratch.reserve(256)) return fail(AQC_ERR_HIP, "hipMalloc failed");
    FrameMeta* d_meta = (FrameMeta*)s->t_scratch.p;
    unsigned long long* d_tot = (unsigned long long*)((uint8_t*)s->t_scratch.p + 64);
    // 1. text to the device; line index in one pass (text_index_kernel): both files in one launch.  The text sits
    //    TEXT_FRONT bytes into its buffer: the writer's 16-byte windows may start a few bytes before a piece's source.
    uint64_t tiles[2] = {0, 0}, cap[2] = {0, 0};
    uint8_t* tbase[2] = {nullptr, nullptr};
    for (int k = 0; k < nf; k++) {
        const size_t slack = IDX_TILE + 64;
        if (arena[k]->reserve(TEXT_FRONT + bytes[k] + slack)) return fail(AQC_ERR_HIP, "hipMalloc of %llu bytes failed", (unsigned long long)bytes[k]);
        tbase[k] = (uint8_t*)arena[k]->p + TEXT_FRONT;
        if (!resident && fx && fx->n[k]) {
            // parts of the chunk are in this device's memory already (aqc_frame_mixed): those move inside HBM, the rest comes up
            uint64_t cur = 0;
            for (uint64_t e = 0; e < fx->n[k]; ++e) {
                const aqc_text_extent& x = fx->ext[k][e];
                if (x.offset < cur || x.offset + x.bytes > bytes[k] || !x.device_text) return fail(AQC_ERR_ARG, "aqc_frame_mixed: extents must be sorted, disjoint and inside the chunk");
                if (x.offset > cur) HIP_TRY(hipMemcpyAsync(tbase[k] + cur, text[k] + cur, x.offset - cur, hipMemcpyHostToDevice, s->stream));
                if (x.bytes) HIP_TRY(hipMemcpyAsync(tbase[k] + x.offset, x.device_text, x.bytes, hipMemcpyDeviceToDevice, s->stream));
                cur = x.offset + x.bytes;
            }
            if (bytes[k] > cur) HIP_TRY(hipMemcpyAsync(tbase[k] + cur, text[k] + cur, bytes[k] - cur, hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemsetAsync(tbase[k] + bytes[k], 0, slack, s->stream));
            s->last_byte[k] = bytes[k] ? fx->last[k] : (uint8_t)'\n';
        } else if (!resident) {
            if (bytes[k]) HIP_TRY(hipMemcpyAsync(tbase[k], text[k], bytes[k], hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemsetAsync(tbase[k] + bytes[k], 0, slack, s->stream));
            s->last_byte[k] = bytes[k] ? text[k][bytes[k] - 1] : (uint8_t)'\n';
        }
        tiles[k] = bytes[k] ? (bytes[k] + IDX_TILE - 1) / IDX_TILE : 1;
        // FASTQ lines average ~90 bytes; a chunk with more lines than this guess is indexed again with the exact size
        const uint64_t guess = bytes[k] / 16 + 4096;
        cap[k] = s->t_line_end[k].cap / sizeof(uint32_t) > guess + 2 ? s->t_line_end[k].cap / sizeof(uint32_t) - 2 : guess;
        if (s->t_line_end[k].reserve(sizeof(uint32_t) * (cap[k] + 2))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    }
    const uint64_t all_tiles = tiles[0] + (paired ? tiles[1] : 0);
    if (s->t_tile[0].reserve(sizeof(unsigned long long) * (all_tiles + 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    // 2. ... the four lines of every complete group, the lock-step record count, the bytes consumed: all queued behind the index
    //    pass without asking the host for anything — the kernels read the line totals where the index pass left them, their grids
    //    are sized for the most lines the chunk could hold.  ONE copy back (FrameOut), ONE wait per chunk.
    const FrameMeta init{0xffffffffu, 0u, 0xffffffffu, 0u};
    FrameMeta h_meta[2] = {init, init};
    FrameOut fo{};
    FrameOut* d_out = (FrameOut*)((uint8_t*)s->t_scratch.p + 128);
    uint32_t virt[2] = {0, 0};
    for (int k = 0; k < nf; k++)      // an unterminated last line of the file is a line (readline() returns it); it may end in blanks
        if (final_[k] && bytes[k] > 0 && s->last_byte[k] != '\n') virt[k] = (uint32_t)bytes[k] | LINE_WS;
    const bool bubble = c->has_cfg && c->cfg.debubble;
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIP_TRY(hipMemsetAsync(s->t_tile[0].p, 0, sizeof(unsigned long long) * (all_tiles + 1), s->stream));
        IndexFile f[2] = {};
        uint32_t t0 = 0;
        for (int k = 0; k < nf; k++) {
            f[k] = IndexFile{(const uint8_t*)tbase[k], bytes[k], (uint32_t*)s->t_line_end[k].p, cap[k], d_tot + k, t0, (uint32_t)tiles[k]};
            t0 += (uint32_t)tiles[k];
        }
        hipLaunchKernelGGL(text_index_kernel, dim3((unsigned)all_tiles), dim3(TXT_BLOCK), 0, s->stream, f[0], f[1],
                           (unsigned long long*)s->t_tile[0].p, (unsigned int*)((unsigned long long*)s->t_tile[0].p + all_tiles));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(d_meta, h_meta, sizeof(h_meta), hipMemcpyHostToDevice, s->stream));
        uint64_t rec_cap = 0;
        for (int k = 0; k < nf; k++) {
            const uint64_t m = (cap[k] + 1) / 4 + 1;            // records the line table could describe
            rec_cap = std::max(rec_cap, m);
            if (seq_off[k]->reserve(4 * m) || qual_off[k]->reserve(4 * m) || seq_len[k]->reserve(4 * m) || s->t_name_off[k].reserve(4 * m) ||
                s->t_name_len[k].reserve(4 * m) || s->t_plus_off[k].reserve(4 * m) || s->t_plus_len[k].reserve(4 * m) ||
                s->t_qual_len[k].reserve(4 * m))
                return fail(AQC_ERR_HIP, "hipMalloc failed");
            FramedFile ff{(uint32_t*)seq_off[k]->p, (uint32_t*)qual_off[k]->p, (uint32_t*)seq_len[k]->p, (uint32_t*)s->t_name_off[k].p,
                          (uint32_t*)s->t_name_len[k].p, (uint32_t*)s->t_plus_off[k].p, (uint32_t*)s->t_plus_len[k].p,
                          (uint32_t*)s->t_qual_len[k].p};
            hipLaunchKernelGGL(frame_records_kernel, dim3((unsigned)((m + TXT_BLOCK - 1) / TXT_BLOCK)), dim3(TXT_BLOCK), 0, s->stream,
                               (const uint8_t*)tbase[k], (const uint32_t*)s->t_line_end[k].p, (const unsigned long long*)(d_tot + k), virt[k], ff, d_meta + k, (uint64_t)cap[k]);
        }
        hipLaunchKernelGGL(frame_finish_kernel, dim3(1), dim3(1), 0, s->stream, (const unsigned long long*)d_tot, (const FrameMeta*)d_meta,
                           (const uint32_t*)s->t_line_end[0].p, (const uint32_t*)(paired ? s->t_line_end[1].p : s->t_line_end[0].p), (const uint32_t*)s->len1.p,
                           virt[0], virt[1], (unsigned long long)bytes[0], (unsigned long long)bytes[1], nf, (unsigned long long)ch->max_records, d_out,
                           (unsigned long long)cap[0], (unsigned long long)cap[1]);
        if (bubble) {
            // lane / tile / x / y out of the R1 names (preprocesser.py:180-192) for the bubble filter
            for (int k = 0; k < 5; k++)
                if (s->aux[k].reserve((k < 4 ? sizeof(int32_t) : 1) * rec_cap)) return fail(AQC_ERR_HIP, "hipMalloc failed");
            hipLaunchKernelGGL(parse_names_kernel, dim3((unsigned)((rec_cap + TXT_BLOCK - 1) / TXT_BLOCK)), dim3(TXT_BLOCK), 0, s->stream,
                               (const uint8_t*)tbase[0], (const uint32_t*)s->t_name_off[0].p, (const uint32_t*)s->t_name_len[0].p, (const unsigned long long*)&d_out->n,
                               (int32_t*)s->aux[0].p, (int32_t*)s->aux[1].p, (int32_t*)s->aux[2].p, (int32_t*)s->aux[3].p,
                               (uint8_t*)s->aux[4].p);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&fo, d_out, sizeof(fo), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(slot_sync(*s));
        // FASTQ lines average ~90 bytes; a chunk with more lines than the table was sized for (counted, not written) is done again
        bool fits = true;
        for (int k = 0; k < nf; k++) {
            const uint64_t real = fo.lines[k] - (virt[k] ? 1 : 0);
            if (real > cap[k]) {
                fits = false;
                cap[k] = real;
                if (s->t_line_end[k].reserve(sizeof(uint32_t) * (cap[k] + 2))) return fail(AQC_ERR_HIP, "hipMalloc failed");
            }
        }
        if (fits) break;
    }
    // 3. lock-step record count (preprocesser.py:412-429)
    // (a record whose quality line is not as long as its sequence line is a record like any other: fastq.py:37-49 does not look,
    //  and every later stage keeps a view per string — LEN_IRR in aqc_batch.hpp)
    const uint64_t n = fo.n;
    memset(info, 0, sizeof(*info));
    info->n = n;
    info->avail1 = fo.avail[0];
    info->avail2 = fo.avail[1];
    info->eof1 = (int32_t)fo.eof[0];
    info->eof2 = paired ? (int32_t)fo.eof[1] : 0;
    info->max_len = fo.max_len;
    // 4. slot view: the text IS the arena, every kernel reads the records in place
    DevBatch v{};
    v.n = n;
    v.first_index = ch->first_index;
    v.seq1 = v.qual1 = (const uint8_t*)tbase[0];
    v.off1 = (const uint32_t*)s->off1.p; v.qoff1 = (const uint32_t*)s->qoff1.p; v.len1 = (const uint32_t*)s->len1.p;
    if (paired) {
        v.seq2 = v.qual2 = (const uint8_t*)tbase[1];
        v.off2 = (const uint32_t*)s->off2.p; v.qoff2 = (const uint32_t*)s->qoff2.p; v.len2 = (const uint32_t*)s->len2.p;
    }
    if (s->results.reserve(sizeof(aqc_result) * (n ? n : 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
    {
        // the quality lines' own lengths (frame_records_kernel) and room for the final quality views of the marked records
        // (written by the verdict kernels for those records only: no traffic for a regular chunk)
        const bool any_irr = fo.first_mismatch[0] < n || (paired && fo.first_mismatch[1] < n);
        s->has_irregular = any_irr;
        for (int k = 0; k < nf; k++)
            if (any_irr && s->qview[k].reserve(sizeof(uint32_t) * (n ? n : 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
        v.qlen1 = (const uint32_t*)s->t_qual_len[0].p; v.qview1 = (uint32_t*)s->qview[0].p;
        v.qlen2 = paired ? (const uint32_t*)s->t_qual_len[1].p : v.qlen1; v.qview2 = paired ? (uint32_t*)s->qview[1].p : v.qview1;
    }
    if (bubble) {
        v.aux_lane = (const int32_t*)s->aux[0].p; v.aux_tile = (const int32_t*)s->aux[1].p;
        v.aux_x = (const int32_t*)s->aux[2].p; v.aux_y = (const int32_t*)s->aux[3].p; v.aux_ok = (const uint8_t*)s->aux[4].p;
    }
    s->view = v;
    s->n = n;
    s->paired = paired;
    s->raw_max_len = info->max_len;
    s->max_len = info->max_len;
    // 5. bytes consumed by the n records (+ R1's next sequence length for the TOTAL_BASES quirk)
    const uint64_t consumed[2] = {fo.consumed[0], fo.consumed[1]};
    const uint32_t h_next = fo.next_len1;
    info->consumed1 = consumed[0];
    info->consumed2 = consumed[1];
    s->consumed[0] = consumed[0]; s->consumed[1] = consumed[1];
    info->next_len1 = h_next;
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
    FormatView v{};
    v.paired = s->paired ? 1 : 0;
    v.results = (const aqc_result*)vs->results.p;
    v.plain = plain ? 1 : 0;
    v.verdict_paired = vs->paired ? 1 : 0;
    v.barcode = c->cfg.barcode ? 1 : 0;
    v.barcode_length = c->cfg.barcode_length;
    v.store_overlap = (store_overlap && vs->paired) ? 1 : 0;
    v.spans = (spans && !plain) ? 1 : 0;
    v.consumed[0] = (uint32_t)s->consumed[0]; v.consumed[1] = (uint32_t)s->consumed[1];
    v.n_framed = s->n;
    s->n_events[0] = s->n_events[1] = 0;
    const DevBuf* sl[2] = {&s->len1, &s->len2};
    const DevBuf* arena[2] = {&s->seq1, &s->seq2};
    const DevBuf* so[2] = {&s->off1, &s->off2};
    const DevBuf* qo[2] = {&s->qoff1, &s->qoff2};
    for (int k = 0; k < (s->paired ? 2 : 1); k++) {
        v.f[k].text = (const uint8_t*)arena[k]->p + TEXT_FRONT;
        v.f[k].seq_off = (const uint32_t*)so[k]->p;
        v.f[k].qual_off = (const uint32_t*)qo[k]->p;
        v.f[k].seq_len = (const uint32_t*)sl[k]->p;
        v.f[k].name_off = (const uint32_t*)s->t_name_off[k].p;
        v.f[k].name_len = (const uint32_t*)s->t_name_len[k].p;
        v.f[k].plus_off = (const uint32_t*)s->t_plus_off[k].p;
        v.f[k].plus_len = (const uint32_t*)s->t_plus_len[k].p;
        v.f[k].qual_len = (const uint32_t*)s->t_qual_len[k].p;
        v.f[k].qview = (const uint32_t*)s->qview[k].p;
    }
    // streams q = file * 3 + {0 good, 1 bad, 2 overlap}: per-tile byte sums -> tile bases (one launch each), the
    // per-record offsets are formed inside the writer
    const uint64_t n_tiles = n ? (n + FMT_TILE - 1) / FMT_TILE : 1;
    const uint64_t n_super = (n_tiles + FMT_SUPER - 1) / FMT_SUPER;
    bool live[6];
    for (int q = 0; q < 6; q++) live[q] = (q < 3 || s->paired) && (q % 3 != 2 || v.store_overlap);
    unsigned long long h_tot[FMT_STREAMS] = {0, 0, 0, 0, 0, 0, 0, 0};
    // the verdict kernel may have done the placement already (AQC_FUSED=1, all n records of the slot, the two-stream case): its totals
    // stand in for the sums / bases passes — unless it gave the placement up (a deferred pair, a record that is not plain text)
    if (s->fused && !plain && !spans && !v.store_overlap && n == s->n && n > 0) {
        unsigned long long misc[5];
        HIP_TRY(hipMemcpyAsync(misc, s->fz_misc.p, sizeof(misc), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        if ((misc[0] >> 32) == 0) {
            v.fused = 1;
            v.fstate[0] = (const uint32_t*)s->fz_rec[0].p; v.fstate[1] = (const uint32_t*)s->fz_rec[1].p;
            v.fbatch = (const unsigned long long*)s->fz_state.p;
            v.fbatch_shift = 5;
            static_assert(FastWaveLds<10, true, true>::PPW == 32, "fbatch_shift");
            h_tot[0] = misc[1]; h_tot[3] = misc[2]; h_tot[1] = misc[3]; h_tot[4] = misc[4];
        }
    }
    if (!v.fused) {
        s->fused = false;          // (whatever this call writes into the good streams replaces what the verdict kernel left there)
        // f_tile: [FMT_STREAMS x n_tiles] the tiles' prefixes inside their super-tiles | [FMT_STREAMS x n_super] the super-tiles' sums -> bases
        if (s->f_tile.reserve(sizeof(unsigned long long) * FMT_STREAMS * (n_tiles + n_super)) || s->t_scratch.reserve(256))
            return fail(AQC_ERR_HIP, "hipMalloc failed");
        unsigned long long* d_tot = (unsigned long long*)((uint8_t*)s->t_scratch.p + 128);
        unsigned long long* d_super = (unsigned long long*)s->f_tile.p + FMT_STREAMS * n_tiles;
        if (n) hipLaunchKernelGGL(fmt_tile_sums_kernel, dim3((unsigned)n_super), dim3(TXT_BLOCK), 0, s->stream, v, n, n_tiles, n_super, (unsigned long long*)s->f_tile.p, d_super);
        else HIP_TRY(hipMemsetAsync(s->f_tile.p, 0, sizeof(unsigned long long) * FMT_STREAMS * (n_tiles + n_super), s->stream));
        hipLaunchKernelGGL(fmt_tile_bases_kernel, dim3(v.spans ? FMT_STREAMS : 6), dim3(TXT_BLOCK), 0, s->stream, d_super, n_super, d_tot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_tot, d_tot, sizeof(unsigned long long) * (v.spans ? FMT_STREAMS : 6), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    if (v.spans) {
        for (int f = 0; f < (s->paired ? 2 : 1); ++f) {
            s->n_events[f] = h_tot[FMT_EVENT_STREAM + f];
            if (s->f_events[f].reserve(sizeof(SpanEvent) * (s->n_events[f] + 1))) return fail(AQC_ERR_HIP, "hipMalloc failed");
        }
    }
    FormatOut outs{};
    for (int q = 0; q < 6; q++) {
        s->f_bytes[q] = live[q] ? h_tot[q] : 0;
        bytes_out[q] = s->f_bytes[q];
        if (s->f_out[q].reserve(s->f_bytes[q] + 64)) return fail(AQC_ERR_HIP, "hipMalloc failed");
        outs.p[q] = (uint8_t*)s->f_out[q].p;
    }
    if (n) {
        const uint64_t n_tasks = n * (s->paired ? 2 : 1);
        // 48-byte plans, (sparse) full piece lists for the records that do not fit a plan, and the list of the records the
        // general copy kernel takes (+ its length)
        const uint64_t gen_cap = ((n_tiles + GEN_LISTS - 1) / GEN_LISTS) * FMT_TILE * (s->paired ? 2 : 1);     // worst case: every record
        // plans: one 16-byte word per (record, file), dense; the six words of the records the general kernel takes, in list order
        const uint64_t plan0_bytes = (16 * n_tasks + 255) / 256 * 256;
        if (s->f_plan.reserve(plan0_bytes + 16 * PLAN_Q * gen_cap * GEN_LISTS) || s->f_patch.reserve(16 * n_tasks + 32 * gen_cap * GEN_LISTS) || s->f_over.reserve(sizeof(FmtTask) * n_tasks) ||
            s->f_pos.reserve(4 * gen_cap * GEN_LISTS + 2 * sizeof(unsigned int) * GEN_LISTS + 64))
            return fail(AQC_ERR_HIP, "hipMalloc failed");
        // f_pos: the general kernel's lists | the lengths of those and of the lists of one-piece plans of a spans / fused format;
        // f_patch: the patch words of the dense plan0 | those listed plans (two words each, in list order)
        uint4* d_wplan = (uint4*)((uint8_t*)s->f_patch.p + 16 * n_tasks);
        unsigned int* d_ngen = (unsigned int*)((uint8_t*)s->f_pos.p + 4 * gen_cap * GEN_LISTS);
        unsigned int* d_nwhole = d_ngen + GEN_LISTS;
        const bool sparse = v.spans || v.fused;
        unsigned copy_blocks = (unsigned)((n_tasks + (COPY_BLOCK / 32) * FMT_UNROLL - 1) / ((COPY_BLOCK / 32) * FMT_UNROLL));
        for (int pass = 0; pass < (v.store_overlap ? 2 : 1); ++pass) {
            HIP_TRY(hipMemsetAsync(d_ngen, 0, 2 * sizeof(unsigned int) * GEN_LISTS, s->stream));
            // GEN_LISTS x k workgroups; k from the worst case, at most 32 per list
            uint64_t per_list = (gen_cap + GEN_ROUND - 1) / GEN_ROUND;
            if (per_list > 32) per_list = 32;
            if (per_list < 1) per_list = 1;
            // text mode without barcodes, main pass (round 6): place + copy in one kernel, piece lists only for the listed records
            // (AQC_PLACE_COPY=0: the plan / whole-copy pair of rounds 2 - 5, for A/B measurements)
            static const bool place_copy = [] { const char* e = getenv("AQC_PLACE_COPY"); return !(e && e[0] == '0'); }();
            if (place_copy && !sparse && pass == 0 && !v.plain && !v.barcode) {
                const unsigned long long* tb = (const unsigned long long*)s->f_tile.p;
                uint4* const pg = (uint4*)((uint8_t*)s->f_plan.p + plan0_bytes);
                hipLaunchKernelGGL(fmt_place_copy_kernel, dim3((unsigned)n_tiles), dim3(PC_BLOCK), 0, s->stream, v, n, n_tiles, n_super, tb, tb + FMT_STREAMS * n_tiles,
                                   pg, (uint32_t*)s->f_pos.p, d_ngen, gen_cap, outs);
                hipLaunchKernelGGL(fmt_plan_listed_kernel, dim3((unsigned)(GEN_LISTS * per_list)), dim3(FMT_TILE), 0, s->stream, v, pg, (FmtTask*)s->f_over.p,
                                   (const uint32_t*)s->f_pos.p, (const unsigned int*)d_ngen, gen_cap, s->status);
            } else {
            hipLaunchKernelGGL(fmt_plan_kernel, dim3((unsigned)n_tiles), dim3(FMT_TILE), 0, s->stream, v, n, n_tiles, n_super,
                               (const unsigned long long*)s->f_tile.p, (const unsigned long long*)s->f_tile.p + FMT_STREAMS * n_tiles, pass, s->status, (uint4*)s->f_plan.p, (uint4*)s->f_patch.p,
                               (uint4*)((uint8_t*)s->f_plan.p + plan0_bytes), (FmtTask*)s->f_over.p, (uint32_t*)s->f_pos.p, d_ngen, gen_cap, d_wplan, d_nwhole, outs.p[0], outs.p[3],
                               (SpanEvent*)s->f_events[0].p, (SpanEvent*)s->f_events[1].p);
            // (spans / fused mode: what stays in the caller's chunk / what the verdict kernel copied has no plan; the records that are their
            //  own bytes but for the walk's byte patches are still this kernel's)
            // (a barcode run has no one-piece record: fmt_plan_kernel writes no dense plans and nothing walks them)
            if (!sparse) {
                if (!(v.barcode && !v.plain)) hipLaunchKernelGGL(fmt_copy_whole_kernel, dim3(copy_blocks), dim3(COPY_BLOCK), 0, s->stream, v, n_tasks, (const uint4*)s->f_plan.p,
                                                                 (const uint4*)s->f_patch.p, outs);
            } else hipLaunchKernelGGL(fmt_copy_whole_list_kernel, dim3((unsigned)(GEN_LISTS * per_list)), dim3(COPY_BLOCK), 0, s->stream, v, (const uint4*)d_wplan, outs,
                                    (const unsigned int*)d_nwhole, gen_cap);
            }
            hipLaunchKernelGGL(fmt_copy_kernel, dim3((unsigned)(GEN_LISTS * per_list)), dim3(COPY_BLOCK), 0, s->stream, v,
                               (const uint4*)((uint8_t*)s->f_plan.p + plan0_bytes), (const FmtTask*)s->f_over.p, outs, (const uint32_t*)s->f_pos.p,
                               (const unsigned int*)d_ngen, gen_cap);
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
    n_events[0] = c->slots[slot].n_events[0];
    n_events[1] = c->slots[slot].n_events[1];
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
        if (n == s->n) { end[f] = s->consumed[f]; continue; }
        uint32_t off = 0;               // record n begins where record n - 1 ends
        HIP_TRY(hipMemcpyAsync(&off, (const uint32_t*)s->t_name_off[f].p + n, sizeof(off), hipMemcpyDeviceToHost, s->stream));
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
    const uint64_t ne = s->n_events[file];
    // (this entry counts in events, not bytes, and says so)
    if (ne > cap) return fail(AQC_ERR_ARG, "aqc_fetch_span_events: %llu events do not fit %llu", (unsigned long long)ne, (unsigned long long)cap);
    return fetch_out(*s, s->f_events[file].p, sizeof(SpanEvent) * ne, dst, sizeof(SpanEvent) * ne, "aqc_fetch_span_events");
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
                           v.len1, (const uint32_t*)s->t_name_off[0].p, (const uint32_t*)s->t_name_len[0].p, n, (int)poly_max, v.first_index,
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
