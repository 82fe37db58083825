// aqc_gunzip_ref.hpp — the device gunzip's kernels (aqc_gunzip_dev.hpp) dealt out by plain loops on the CPU.  Host only.
//
// The header's GZB_HD functions are what the kernels' lanes execute: the block-start tests, the table builder, the block
// decoder, the chain walk, the marker re-basing.  CpuOffload deals them out with plain loops in the kernels' order
// (scan -> compact -> decode -> chain -> gather, same buffers, same GzbJob) behind the SectionOffload interface the GPU's
// DeviceInflate has (aqc_gunzip_offload.hip).  Two users: tests/native/gzb_selftest.cpp plugs it into the real ParallelGunzip,
// and aqc_gunzip_probe (engine 0) runs one group and one resolve with it — the reference the kernels are held to, section by
// section.  Its sizing rules default to the selftest's; the probe sets them to DeviceInflate's (slack, sec_ratio).
#pragma once
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "aqc_gunzip_dev.hpp"
#include "aqc_gz.hpp"

namespace aqc {

struct CpuOffload : aqcgz::SectionOffload {
    size_t group;
    uint32_t ratio_cap = 20, tok_ratio = 8, overlap_tokens = 2048;
    uint32_t cand_div = 4096;            // candidate capacity = span / cand_div + 256
    uint32_t slice_tokens = 300, max_slices = 1u << 20;
    // how DeviceInflate::run_group sizes a group, where it differs from the selftest's habits: the compressed bytes taken behind
    // the last stop bit, a section's symbol limit (sec_ratio x its compressed bytes + 2 MiB), and no limit on all sections' symbols
    // together (its result set is made to measure once the sections' sizes are known)
    uint64_t slack = 256u << 10;
    uint32_t sec_ratio = 12;
    bool total_unbounded = false;
    uint64_t groups = 0, sections = 0, found = 0, candidates = 0, false_ends = 0, spec_lanes = 0, failed_blocks = 0, stitched_blocks = 0;
    std::vector<std::vector<uint16_t>*> live;
    std::vector<aqcgz::OffloadResult> pending_results;
    // break_after >= 0: the "device" fails on its (break_after + 1)-th group — the group's sections come back empty, as
    // DeviceInflate hands them back after a HIP error — and takes no work from then on (ready() == false)
    long break_after = -1;
    bool broken = false;
    // resident mode (round 6): the symbols stay "on the device" — a GroupRes — until the consumer asks for the run to be resolved
    // (gzb_window_byte / gzb_resolve_sym / gzb_crc_slot + gzb_crc_join, dealt out the way gzb_windows_kernel, gzb_resolve_kernel
    // and gzb_crc_kernel deal them) and then fetches bytes
    bool resident = false;
    uint64_t runs_resolved = 0, sections_resolved = 0;
    long resolve_breaks_after = -1;       // >= 0: resolve() fails (as after a HIP error) from its (n + 1)-th call on
    struct GroupRes {
        std::vector<uint16_t> sym;
        std::vector<uint8_t> text;
        std::vector<uint64_t> off;
        std::vector<uint32_t> nsym;
    };
    struct ResTok { std::shared_ptr<GroupRes> g; int k; };
    explicit CpuOffload(size_t g) : group(g) {}
    size_t group_bytes() const override { return group; }
    bool ready() override { return !broken; }
    bool gave_up() override { return broken; }
    void release(void* token) override {
        if (resident) delete (ResTok*)token;
        else delete (std::vector<uint16_t>*)token;
    }
    const uint8_t* text_ptr(void* token, int* device) override {
        ResTok* t = (ResTok*)token;
        if (device) *device = 0;
        return t->g->text.data() + t->g->off[t->k];
    }
    int resolve(void* const* tokens, int n, const uint8_t* win, size_t wlen, uint32_t* crc, uint8_t* tail, size_t* tail_len, uint32_t* piece_nl) override {
        if (resolve_breaks_after >= 0 && (long)runs_resolved >= resolve_breaks_after) return -2;
        ++runs_resolved;
        sections_resolved += (uint64_t)n;
        GroupRes& G = *((ResTok*)tokens[0])->g;
        for (int k = 0; k < n; ++k) if (((ResTok*)tokens[k])->g.get() != &G) return -2;
        std::vector<uint64_t> off((size_t)n);
        std::vector<uint32_t> nsym((size_t)n);
        for (int k = 0; k < n; ++k) { const int sk = ((ResTok*)tokens[k])->k; off[k] = G.off[sk]; nsym[k] = G.nsym[sk]; }
        std::vector<uint8_t> wins((size_t)(n + 1) * GZB_WINDOW, 0);
        if (wlen) memcpy(wins.data() + GZB_WINDOW - wlen, win, wlen);
        uint32_t bad = 0;
        GzbResolveJob R{};
        R.sym = G.sym.data(); R.text = G.text.data(); R.wins = wins.data(); R.off = off.data(); R.nsym = nsym.data(); R.n_run = (uint32_t)n;
        R.valid0 = (uint32_t)(GZB_WINDOW - wlen); R.bad = &bad;
        // gzb_windows_kernel
        uint32_t valid = R.valid0;
        std::vector<uint32_t> valids((size_t)n);
        for (int k = 0; k < n; ++k) {
            valids[k] = valid;
            const uint8_t* w = wins.data() + (size_t)k * GZB_WINDOW;
            uint8_t* o = wins.data() + (size_t)(k + 1) * GZB_WINDOW;
            for (uint32_t j = 0; j < GZB_WINDOW; ++j) o[j] = gzb_window_byte(R, (uint32_t)k, j, w, valid, &bad);
            valid = nsym[k] >= valid ? 0u : valid - nsym[k];
        }
        // gzb_resolve_kernel
        for (int k = 0; k < n; ++k) {
            const uint32_t v = gzb_window_valid(R, (uint32_t)k);
            if (v != valids[k]) { printf("gzb_window_valid disagrees with the window pass\n"); return -2; }
            const uint8_t* w = wins.data() + (size_t)k * GZB_WINDOW;
            for (uint32_t i = 0; i < nsym[k]; ++i) G.text[off[k] + i] = gzb_resolve_sym(G.sym[off[k] + i], w, v, &bad);
        }
        if (bad) return aqcgz::GZ_ERR_DATA;
        // gzb_crc_kernel + the host's fold
        static std::vector<uint32_t> tab, adv_piece;
        auto advance = [](uint32_t x, uint64_t len) { return (uint32_t)crc32_combine((uLong)x, 0UL, (z_off_t)len); };
        if (tab.empty()) {
            tab.resize(GZB_CRC_TAB_WORDS);
            gzb_crc_tables(tab.data(), advance);
            adv_piece.resize(32);
            for (int j = 0; j < 32; ++j) adv_piece[j] = advance(1u << j, GZB_CRC_PIECE);
        }
        for (int k = 0; k < n; ++k) {
            const uint32_t cnt = (nsym[k] + GZB_CRC_PIECE - 1u) / GZB_CRC_PIECE;
            std::vector<uint32_t> pieces(cnt);
            for (uint32_t pi = 0; pi < cnt; ++pi) {
                uint32_t part[GZB_CRC_THREADS], lines = 0;
                for (uint32_t t = 0; t < GZB_CRC_THREADS; ++t) { uint32_t lf = 0; part[t] = gzb_crc_slot(G.text.data() + off[k], nsym[k], cnt, pi, t, tab.data(), &lf); lines += lf; }
                if (piece_nl) *piece_nl++ = lines;
                for (int level = 0; level < 8; ++level) {
                    const uint32_t step = 1u << level;
                    for (uint32_t t = 0; t < GZB_CRC_THREADS; t += 2u * step) part[t] = gzb_crc_join(part[t], part[t + step], level, tab.data());
                }
                pieces[pi] = part[0];
            }
            crc[k] = gzb_crc_fold(pieces.data(), cnt, nsym[k], adv_piece.data(), advance);
            if (crc[k] != (uint32_t)crc32(0L, G.text.data() + off[k], nsym[k])) { printf("device CRC of a section differs from zlib's\n"); return -2; }
        }
        uint64_t total = 0;
        for (int k = 0; k < n; ++k) total += nsym[k];
        const size_t tl = (size_t)std::min<uint64_t>(GZB_WINDOW, wlen + total);
        memcpy(tail, wins.data() + (size_t)n * GZB_WINDOW + GZB_WINDOW - tl, tl);
        *tail_len = tl;
        return 0;
    }
    std::vector<std::pair<std::pair<const uint8_t*, uint8_t*>, size_t>> queued;      // fetch(): copies land at fetch_wait(), as a stream's would
    bool fetch(void* token, size_t off, size_t len, uint8_t* dst) override {
        ResTok* t = (ResTok*)token;
        if (off + len > t->g->nsym[t->k]) return false;
        queued.push_back({{t->g->text.data() + t->g->off[t->k] + off, dst}, len});
        return true;
    }
    bool fetch_wait() override {
        for (auto& q : queued) memcpy(q.first.second, q.first.first, q.second);
        queued.clear();
        return true;
    }

    bool submit(const uint8_t* data, size_t size, int n, const uint64_t* nominal, const uint64_t* stop, const uint8_t* exact,
                std::function<void(int, const aqcgz::OffloadResult&)> done) override {
        if (broken) return false;
        if (break_after >= 0 && (long)groups >= break_after) {
            broken = true;
            ++groups;
            aqcgz::OffloadResult none;
            std::thread([n, done, none] { for (int k = 0; k < n; ++k) done(k, none); }).detach();
            return true;
        }
        const uint64_t byte0 = (nominal[0] >> 3) & ~(uint64_t)15;
        const uint64_t end_byte = std::min<uint64_t>(size, (stop[n - 1] >> 3) + 1 + slack);
        const size_t span = (size_t)(end_byte - byte0);
        std::vector<uint8_t> comp(span + 256, 0);
        memcpy(comp.data(), data + byte0, span);
        GzbJob J{};
        J.comp = comp.data(); J.comp_bytes = (uint32_t)span; J.scan_byte0 = 0;
        J.first_bit = (uint32_t)(nominal[0] - byte0 * 8);
        J.last_bit = (uint32_t)std::min<uint64_t>(stop[n - 1] - byte0 * 8, (uint64_t)span * 8);
        J.n_tiles = (uint32_t)(((size_t)(J.last_bit >> 3) + 1 + GZB_SCAN_TILE - 1) / GZB_SCAN_TILE);
        J.cand_cap = (uint32_t)(span / cand_div + 256);
        J.ratio_cap = ratio_cap;
        std::vector<uint32_t> tile_cnt(J.n_tiles), tile_cand((size_t)J.n_tiles * GZB_TILE_CAND), n_cand(2), c_start(J.cand_cap), c_end(J.cand_cap), c_nsym(J.cand_cap),
            c_flags(J.cand_cap), c_symcap(J.cand_cap);
        std::vector<uint64_t> c_symoff(J.cand_cap);
        J.tile_cnt = tile_cnt.data(); J.tile_cand = tile_cand.data(); J.n_cand = n_cand.data(); J.c_start = c_start.data(); J.c_end = c_end.data();
        J.c_nsym = c_nsym.data(); J.c_flags = c_flags.data(); J.c_symcap = c_symcap.data(); J.c_symoff = c_symoff.data();
        J.blk_sym_cap = gzb_sym_budget(span, ratio_cap);
        std::unique_ptr<uint16_t[]> blk_sym(new uint16_t[J.blk_sym_cap + 64]);
        J.blk_sym = blk_sym.get();
        J.tok_ratio = tok_ratio;
        J.overlap_tokens = overlap_tokens;
        J.blk_tp_cap = gzb_tok_budget(span, tok_ratio, overlap_tokens);
        std::unique_ptr<unsigned long long[]> blk_tp(new unsigned long long[J.blk_tp_cap + 64]);
        std::vector<uint64_t> c_tokoff(J.cand_cap);
        std::vector<uint32_t> c_tokcap(J.cand_cap);
        J.c_tokoff = c_tokoff.data(); J.c_tokcap = c_tokcap.data();
        std::vector<uint32_t> c_lanes(J.cand_cap), l_u32((size_t)5 * J.cand_cap * GZB_K);
        J.blk_tp = blk_tp.get(); J.c_lanes = c_lanes.data();
        J.l_p = l_u32.data(); J.l_stop = J.l_p + (size_t)J.cand_cap * GZB_K; J.l_start = J.l_stop + (size_t)J.cand_cap * GZB_K;
        J.l_ntok = J.l_start + (size_t)J.cand_cap * GZB_K; J.l_flags = J.l_ntok + (size_t)J.cand_cap * GZB_K;
        std::vector<uint32_t> tables((size_t)J.cand_cap * GZB_TAB_WORDS);
        J.tables = tables.data();
        // ---- scan: every lane of every tile
        uint8_t kraft[512];
        for (int i = 0; i < 512; ++i) kraft[i] = (uint8_t)gzb_kraft9((uint32_t)i);
        std::vector<uint8_t> cl(128);
        const uint32_t limit_bit = J.comp_bytes * 8u;
        for (uint32_t tile = 0; tile < J.n_tiles; ++tile) {
            std::vector<uint32_t> hits;
            for (uint32_t tid = 0; tid < (uint32_t)GZB_SCAN_THREADS; ++tid) {
                const uint32_t b0 = tile * (uint32_t)GZB_SCAN_TILE + tid * 16u;
                if (b0 >= J.comp_bytes) continue;
                uint32_t d[8];
                memcpy(d, comp.data() + b0, 32);
                for (int i = 0; i < 4; ++i) {
                    const unsigned long long v64 = ((unsigned long long)d[i + 1] << 32) | d[i];
                    uint32_t mm = gzb_quick32(v64);
                    const uint32_t bb = (b0 + 4u * (uint32_t)i) * 8u;
                    if (bb + 32u <= J.first_bit || bb >= J.last_bit) mm = 0;
                    else {
                        if (bb < J.first_bit) mm &= ~0u << (J.first_bit - bb);
                        if (bb + 32u > J.last_bit) mm &= (1u << (J.last_bit - bb)) - 1u;
                    }
                    while (mm) {
                        const uint32_t bit = (uint32_t)__builtin_ctz(mm);
                        mm &= mm - 1;
                        const uint32_t p = bb + bit;
                        const uint32_t hclen = ((uint32_t)(v64 >> (bit + 13u)) & 15u) + 4u;
                        if (!gzb_kraft_ok(comp.data(), p, hclen, kraft)) continue;
                        uint32_t db, hl, hd;
                        if (gzb_header(comp.data(), limit_bit, p, cl.data(), 1, nullptr, db, hl, hd)) hits.push_back(p);
                    }
                }
            }
            std::sort(hits.begin(), hits.end());
            const uint32_t c = (uint32_t)std::min<size_t>(hits.size(), (size_t)GZB_TILE_CAND);
            tile_cnt[tile] = c;
            for (uint32_t a = 0; a < c; ++a) tile_cand[(size_t)tile * GZB_TILE_CAND + a] = hits[a];
        }
        // ---- compact
        uint32_t nc = 0;
        for (uint32_t t = 0; t < J.n_tiles; ++t)
            for (uint32_t a = 0; a < tile_cnt[t]; ++a)
                if (nc < J.cand_cap) c_start[nc++] = tile_cand[(size_t)t * GZB_TILE_CAND + a];
        n_cand[0] = nc; n_cand[1] = 0;
        candidates += nc;
        {
            unsigned long long o = 0, to = 0;
            for (uint32_t c = 0; c < nc; ++c) {
                const uint32_t cap = gzb_symcap_of(J, c, nc), tcap = gzb_tokcap_of(J, c, nc);
                c_symoff[c] = o;
                c_tokoff[c] = to;
                c_tokcap[c] = tcap;
                c_symcap[c] = (o + cap > J.blk_sym_cap || to + tcap > J.blk_tp_cap) ? 0u : cap;
                o += cap;
                to += tcap;
            }
        }
        // ---- decode: tables per candidate, then GZB_K lanes per candidate in slices, then the stitch
        std::vector<uint32_t> cnt(16), nxt(16), off(16);
        for (uint32_t c = 0; c < nc; ++c) {
            uint32_t* const tw = J.tables + (size_t)c * GZB_TAB_WORDS;
            const GzbLaneTab<1> T{reinterpret_cast<uint16_t*>(tw)};
            uint8_t* const lens = reinterpret_cast<uint8_t*>(tw + GZB_TAB_ENTRIES / 2);
            uint32_t p = 0, hlit = 0, hdist = 0, fl = 0;
            if (c_symcap[c] == 0) fl = GZB_F_SKIP;
            else if (!gzb_header(J.comp, limit_bit, c_start[c], cl.data(), 1, lens, p, hlit, hdist)) fl = GZB_F_ERROR;
            if (!fl) {
                gzb_build<true>(lens, hlit, T, cnt.data(), nxt.data(), off.data(), 1);
                gzb_build<false>(lens + hlit, hdist, T, cnt.data(), nxt.data(), off.data(), 1);
                gzb_plan_lanes(J, c, nc, p);
            } else {
                c_lanes[c] = 0;
                for (uint32_t k = 0; k < (uint32_t)GZB_K; ++k) J.l_flags[c * GZB_K + k] = 0;
            }
            c_flags[c] = fl; c_nsym[c] = 0; c_end[c] = 0;
        }
        // in slices, like the kernels: a slice ends after slice_tokens tokens, the next one resumes at the saved bit / token count
        for (uint32_t sl = 0; sl < max_slices; ++sl)
            for (uint32_t i = 0; i < nc * (uint32_t)GZB_K; ++i) {
                const uint32_t c = i / (uint32_t)GZB_K, k = i % (uint32_t)GZB_K;
                if (J.l_flags[i] != GZB_F_MORE) continue;
                const uint32_t lanes = c_lanes[c];
                if (lanes > 1) ++spec_lanes;
                const GzbLaneTab<1> T{reinterpret_cast<uint16_t*>(J.tables + (size_t)c * GZB_TAB_WORDS)};
                const uint32_t share = c_tokcap[c] / (uint32_t)GZB_K;
                const size_t at = c_tokoff[c] + (size_t)k * share;
                uint32_t p = J.l_p[i], nt = J.l_ntok[i];
                GzbInMem in{J.comp, 0};
                J.l_flags[i] = gzb_tokenize(in, limit_bit, T, J.blk_tp + at, lanes == 1u ? share * (uint32_t)GZB_K : share, p, nt, J.l_stop[i], slice_tokens, lanes != 1u);
                J.l_p[i] = p; J.l_ntok[i] = nt;
            }
        for (uint32_t c = 0; c < nc; ++c) {
            if (c_flags[c]) continue;
            uint32_t ns = 0, eb = 0;
            const uint32_t fl = gzb_stitch_expand(J, c, ns, eb);
            c_flags[c] = fl; c_nsym[c] = fl ? 0u : ns; c_end[c] = eb;
            if (fl) ++failed_blocks;
            if (!fl && c_lanes[c] > 1) ++stitched_blocks;
        }
        // ---- chain + gather
        uint64_t sec_max = 0;
        for (int k = 0; k < n; ++k) sec_max = std::max<uint64_t>(sec_max, (stop[k] - nominal[k]) >> 3);
        J.s_symcap = (uint32_t)std::min<uint64_t>((sec_max * sec_ratio + (2u << 20) + 7) & ~(uint64_t)7, 0xfffffff0u);
        J.n_sec = (uint32_t)n;
        std::vector<uint32_t> s_nom(n), s_stop(n), s_exact(n), s_start(n), s_end(n), s_nsym(n), s_nblk(n), s_blocks((size_t)n * GZB_SEC_BLOCKS * 3);
        for (int k = 0; k < n; ++k) {
            s_nom[k] = (uint32_t)(nominal[k] - byte0 * 8);
            s_stop[k] = (uint32_t)std::min<uint64_t>(stop[k] - byte0 * 8, (uint64_t)span * 8);
            s_exact[k] = exact[k];
        }
        J.s_nominal = s_nom.data(); J.s_stop = s_stop.data(); J.s_exact = s_exact.data(); J.s_start = s_start.data(); J.s_end = s_end.data();
        J.s_nsym = s_nsym.data(); J.s_nblk = s_nblk.data(); J.s_blocks = s_blocks.data();
        std::vector<uint64_t> s_off((size_t)n + 1);
        J.s_off = s_off.data();
        J.s_sym_total = total_unbounded ? ~0ull >> 2 : (uint64_t)span * 12 + (uint64_t)n * 64 + (1u << 20);
        ++groups;
        sections += (uint64_t)n;
        for (int k = 0; k < n; ++k) gzb_chain_section(J, (uint32_t)k);
        gzb_place(J);
        std::vector<uint16_t> s_sym(s_off[(size_t)n] + 64);       // (what the sections that chained up need: known only now)
        J.s_sym = s_sym.data();
        std::shared_ptr<GroupRes> res;
        if (resident) {
            res.reset(new GroupRes());
            res->off.assign(s_off.begin(), s_off.begin() + n);
            res->nsym.assign(s_nsym.begin(), s_nsym.end());
        }
        for (int k = 0; k < n; ++k) {
            aqcgz::OffloadResult r;
            if (s_start[k] != GZB_NONE && s_nsym[k] != 0) {
                uint16_t* const dst = s_sym.data() + s_off[k];
                const uint32_t* const blocks = s_blocks.data() + (size_t)k * GZB_SEC_BLOCKS * 3u;
                for (uint32_t b = 0; b < s_nblk[k]; ++b) {
                    const uint32_t w0 = blocks[3u * b], w1 = blocks[3u * b + 1], o = blocks[3u * b + 2];
                    if (w0 & GZB_STORED) { for (uint32_t i = 0; i < (w0 & 0xffffu); ++i) dst[o + i] = comp[w1 + i]; }
                    else {
                        const uint16_t* const s = J.blk_sym + c_symoff[w0];
                        for (uint32_t i = 0; i < c_nsym[w0]; ++i) dst[o + i] = gzb_rebase(s[i], o, dst);
                    }
                }
                r.found = true;
                r.start_bit = byte0 * 8 + s_start[k];
                r.end_bit = byte0 * 8 + s_end[k];
                r.n_sym = s_nsym[k];
                if (!resident) {
                    auto* keep = new std::vector<uint16_t>(dst, dst + s_nsym[k]);
                    r.sym = keep->data();
                    r.token = keep;
                }
                ++found;
            }
            if (!resident) done(k, r);
            else if (r.found) { r.resident = true; r.token = new ResTok{res, k}; }
            if (resident) pending_results.push_back(r);
        }
        if (resident) {
            // (the symbols of all sections are final only now: a later section's gather does not touch an earlier one's, but the
            //  buffer is handed over whole)
            res->sym.assign(s_sym.begin(), s_sym.begin() + (long)s_off[n] + 64);
            res->text.assign((size_t)s_off[n] + 64, 0);
            for (int k = 0; k < n; ++k) done(k, pending_results[(size_t)k]);
            pending_results.clear();
        }
        return true;
    }
};

}  // namespace aqc
