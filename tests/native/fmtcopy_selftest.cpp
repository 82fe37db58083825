// csrc/aqc_fmtwin.hpp on the CPU: the arithmetic of the text writer's forward copies (aqc_fmtcopy.hpp) — the window rule of the
// whole-record copies, the window rule of the general copy kernel, the packing of a piece list into six plan words and what a lane
// reads back from them — compiled without HIP and dealt out by plain loops over the work items, the way the kernels' lanes take them.
//   1. whole records: every length 16 .. 512 at every source alignment: at most 32 windows, none outside the record, together all
//      of it, windows 1 .. n - 2 on the source's 16-byte grid where the rule says so;
//   2. pieces of the general kernel: every length 16 .. 1100 (and 1 .. 15) at every alignment, text and literal: piece_items windows,
//      none outside the piece, together all of it, from GRID_MIN bytes on each on the grid or end-aligned;
//   3. plans: random piece lists of 1 .. 8 pieces with lengths around every edge, packed by plan_words and decoded per work item,
//      against a linear search; lists that do not fit a plan (9 pieces, 65 work items, 5 patches, a patch in a short piece) are refused.
// Every copy goes through the windows, byte by byte, into a heap block that ENDS with the record or piece (the source block ends
// with it too), so that any access behind is an ASan report; the bytes must be the source's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_fmtwin.hpp"

using namespace aqc;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static void fill(uint8_t* p, uint32_t n) { for (uint32_t i = 0; i < n; ++i) p[i] = (uint8_t)(rnd() % 251u + 1u); }

// ---- 1. copy_whole_tasks ---------------------------------------------------------------------------------------------------------
static uint64_t whole_record(uint32_t align, int len) {
    std::vector<uint8_t> sblk(16 + align + (uint32_t)len);
    uint8_t* src = sblk.data();
    src += ((16 - ((uintptr_t)src & 15)) & 15) + align;
    fill(src, (uint32_t)len);
    uint8_t* dst = (uint8_t*)malloc((size_t)len);       // ends with the record
    memset(dst, 0, (size_t)len);
    const int a = (16 - (int)align) & 15;               // bytes to the source's next boundary
    const int n_grid = 1 + (len - a + 15) / 16, n_plain = (len + 15) / 16;
    const bool grid = a != 0 && n_grid <= 32;
    std::vector<int> covered((size_t)len, 0);
    const int nw = whole_window(len, src, 0).nw;
    CHECK(nw == (grid ? n_grid : n_plain), "window count: len %d align %u -> %d", len, align, nw);
    CHECK(nw >= 1 && nw <= 32, "more than 32 windows: len %d align %u -> %d", len, align, nw);
    for (int lane = 0; lane < 32; ++lane) {
        const WholeWin w = whole_window(len, src, lane);
        CHECK(w.nw == nw, "window count depends on the lane: len %d align %u lane %d", len, align, lane);
        CHECK(w.off >= 0 && w.off + 16 <= len, "window outside the record: len %d align %u lane %d off %d", len, align, lane, w.off);
        if (lane >= nw) continue;
        if (lane == 0) CHECK(w.off == 0, "lane 0 does not take the record's start: len %d align %u off %d", len, align, w.off);
        if (grid && lane >= 1 && lane + 1 < nw) CHECK(((align + (uint32_t)w.off) & 15u) == 0, "window off the grid: len %d align %u lane %d off %d", len, align, lane, w.off);
        if (!grid && lane + 1 < nw) CHECK(w.off == 16 * lane, "plain window: len %d align %u lane %d off %d", len, align, lane, w.off);
        if (lane + 1 == nw) CHECK(w.off + 16 == len, "the last window does not end with the record: len %d align %u off %d", len, align, w.off);
        for (int i = 0; i < 16; ++i) { dst[w.off + i] = src[w.off + i]; covered[(size_t)(w.off + i)]++; }
    }
    for (int i = 0; i < len; ++i) CHECK(covered[(size_t)i] > 0, "byte %d of a record of %d not written (align %u)", i, len, align);
    CHECK(memcmp(dst, src, (size_t)len) == 0, "bytes differ: len %d align %u", len, align);
    free(dst);
    return (uint64_t)nw;
}

// ---- 2. the general kernel's pieces ---------------------------------------------------------------------------------------------
// the bytes a lane writes for work item d of a piece: a 16-byte window, or all of a short piece (8 + 4 + 2 + 1 by the bits of its length)
static void copy_item(uint8_t* dst, const uint8_t* src, int lk, int off, std::vector<int>* covered, int base) {
    const int nb = lk >= 16 ? 16 : lk;
    if (lk < 16) {
        // the kernel's stores for a short piece: 8 bytes at 0, 4 at (lk & 8), 2 at (lk & 12), 1 at (lk & 14)
        int at = 0;
        for (int bit = 8; bit; bit >>= 1)
            if (lk & bit) { memcpy(dst + at, src + at, (size_t)bit); at += bit; }
        CHECK(at == lk, "short piece of %d bytes: %d stored", lk, at);
    } else memcpy(dst + off, src + off, 16);
    if (covered) for (int i = 0; i < nb; ++i) (*covered)[(size_t)(base + off + i)]++;
}

static uint64_t general_piece(uint32_t align, int lk, bool literal) {
    std::vector<uint8_t> sblk(16 + align + (uint32_t)lk);
    uint8_t* src = sblk.data();
    src += ((16 - ((uintptr_t)src & 15)) & 15) + align;
    fill(src, (uint32_t)lk);
    uint8_t* dst = (uint8_t*)malloc((size_t)lk);
    memset(dst, 0, (size_t)lk);
    // the text's base and the piece's offset in it: only their sum's low bits count; split them differently from piece to piece
    const uint32_t split = rnd() & 0xffffu;
    const uint32_t tbase = (uint32_t)(uintptr_t)src - split;
    const uint32_t sk = literal ? (FMT_LIT_BIT | (rnd() % 14u) * 16u) : split;
    const int items = (int)piece_items((uint32_t)lk);
    const bool grid = lk >= (int)GRID_MIN && !literal;
    CHECK(items == (lk < 16 ? 1 : (lk + 15) / 16 + (lk >= 48 ? 1 : 0)), "piece_items(%d) = %d", lk, items);
    std::vector<int> covered((size_t)lk, 0);
    for (int d = 0; d < items; ++d) {
        const int off = gen_window_off(lk, tbase, sk, d);
        if (lk < 16) { CHECK(off == 0, "short piece: lk %d off %d", lk, off); }
        else CHECK(off >= 0 && off + 16 <= lk, "window outside the piece: lk %d align %u item %d off %d", lk, align, d, off);
        if (d == 0) CHECK(off == 0, "item 0 does not take the piece's start: lk %d align %u", lk, align);
        // (piece_items is the count of the worst alignment: at others the last two items both end with the piece)
        if (grid && d >= 1 && d + 1 < items) CHECK(((align + (uint32_t)off) & 15u) == 0 || off + 16 == lk, "window off the grid: lk %d align %u item %d off %d", lk, align, d, off);
        if (!grid && lk >= 16) CHECK(off == (16 * d < lk - 16 ? 16 * d : lk - 16), "plain window: lk %d item %d off %d", lk, d, off);
        if (lk >= 16 && d + 1 == items) CHECK(off + 16 == lk, "the last window does not end with the piece: lk %d align %u off %d", lk, align, off);
        copy_item(dst, src, lk, off, &covered, 0);
    }
    for (int i = 0; i < lk; ++i) CHECK(covered[(size_t)i] > 0, "byte %d of a piece of %d not written (align %u)", i, lk, align);
    CHECK(memcmp(dst, src, (size_t)lk) == 0, "bytes differ: lk %d align %u", lk, align);
    free(dst);
    return (uint64_t)items;
}

// ---- 3. plans ---------------------------------------------------------------------------------------------------------------------
static const int LENS[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 47, 48, 49, 200};

struct Made { FmtTask t; uint32_t text_bytes; };
static Made make_task(int np, int n_patch, bool patch_in_short) {
    Made m;
    memset(&m.t, 0, sizeof(m.t));
    FmtTask& t = m.t;
    t.stream = (uint8_t)(rnd() % 3u);
    t.np = (uint8_t)np;
    uint32_t o = 0, items = 0, text = 64 + rnd() % 16u;
    for (int k = 0; k < np && k < FMT_MAXP; ++k) {
        const int len = LENS[rnd() % (sizeof(LENS) / sizeof(LENS[0]))];
        const bool lit = len <= 12 && rnd() % 4u == 0;
        t.p[k].src = lit ? (FMT_LIT_BIT | (rnd() % 14u) * 16u) : text;
        t.p[k].dst = (uint16_t)o;
        t.p[k].len = (uint16_t)len;
        text += (uint32_t)len + 1 + rnd() % 5u;          // (a gap: neighbours in the text would have been merged)
        o += (uint32_t)len;
        items += piece_items((uint32_t)len);
    }
    t.total = (uint16_t)o;
    t.items = (uint16_t)items;
    m.text_bytes = text + 32;
    for (int e = 0; e < n_patch; ++e) {
        // a position inside a piece of >= 16 bytes (or, asked for, inside a short one)
        for (int tries = 0; tries < 200; ++tries) {
            const int k = (int)(rnd() % (uint32_t)(np < FMT_MAXP ? np : FMT_MAXP));
            if ((t.p[k].len < 16) != (patch_in_short && e == 0)) continue;
            t.patch[t.n_patch++] = ((uint32_t)t.p[k].dst + rnd() % t.p[k].len) | ((33u + rnd() % 40u) << 16);
            break;
        }
    }
    return m;
}

static bool has_piece(const FmtTask& t, bool short_one) {
    for (int k = 0; k < t.np && k < FMT_MAXP; ++k) if ((t.p[k].len < 16) == short_one) return true;
    return false;
}

// one plan: pack, decode every work item against a linear search, copy through the windows; -> 1 when the list fits a plan
static int one_plan(const Made& m, uint64_t& items_seen) {
    const FmtTask& t = m.t;
    const uint32_t pos = rnd();
    const PlanWords pw = plan_words(t, pos);
    alignas(16) uint8_t pb[16 * PLAN_Q];
    const uint4 q[PLAN_Q] = {pw.q0, pw.q1, pw.q2, pw.q3, pw.q4, pw.q5};
    memcpy(pb, q, sizeof(pb));
    bool patch_short = false;
    for (int e = 0; e < t.n_patch; ++e)
        for (int k = 0; k < t.np && k < FMT_MAXP; ++k)
            if ((t.patch[e] & 0xffffu) >= t.p[k].dst && (t.patch[e] & 0xffffu) < (uint32_t)t.p[k].dst + t.p[k].len && t.p[k].len < 16) patch_short = true;
    const bool fits = t.np <= 8 && t.n_patch <= 4 && t.items <= 64 && !patch_short;
    CHECK(pw.inline_ok == fits, "inline_ok %d, want %d: np %d patches %d items %d", (int)pw.inline_ok, (int)fits, t.np, t.n_patch, t.items);
    CHECK(pw.q0.x == pos, "q0.x is not the record's place");
    if (!pw.inline_ok) {
        CHECK(pw.q0.y == (PLAN_OVER | t.stream), "an overflow plan's q0.y: %08x", pw.q0.y);
        CHECK(!plan_is_whole(pw.q0), "an overflow plan passes for a whole record");
        return 0;
    }
    CHECK((pw.q0.y & 0xffu) == t.stream && ((pw.q0.y >> 8) & 0xffu) == t.np && ((pw.q0.y >> 16) & 0xffu) == t.n_patch && !(pw.q0.y & PLAN_OVER), "q0.y %08x", pw.q0.y);
    const uint32_t pt[4] = {pw.q5.x, pw.q5.y, pw.q5.z, pw.q5.w};
    for (int e = 0; e < 4; ++e) CHECK(pt[e] == (e < t.n_patch ? t.patch[e] : 0u), "patch word %d", e);
    // the whole-record copy takes exactly the one-piece plans of 16 .. 512 text bytes
    CHECK(plan_is_whole(pw.q0) == (t.np == 1 && !(t.p[0].src & FMT_LIT_BIT) && t.p[0].len >= 16 && t.p[0].len <= 512), "plan_is_whole: np %d len %d", t.np, t.p[0].len);
    // the text the pieces come from, the literal table, and an output block that ends with the record
    std::vector<uint8_t> text(m.text_bytes + 16), lit(16 * 16 + 16);
    fill(text.data(), (uint32_t)text.size());
    fill(lit.data(), (uint32_t)lit.size());
    uint8_t* out = (uint8_t*)malloc(t.total);
    memset(out, 0, t.total);
    std::vector<int> covered(t.total, 0);
    for (uint32_t item = 0; item < t.items; ++item) {
        const PlanPiece pc = plan_piece_of(pb, item);
        int k = 0;
        uint32_t first = 0;
        while (first + piece_items(t.p[k].len) <= item) { first += piece_items(t.p[k].len); ++k; }
        CHECK(pc.items == t.items, "total items %u, want %u", pc.items, t.items);
        CHECK(pc.k == k && pc.first_item == (int)first && pc.lk == (int)t.p[k].len && pc.dst_off == (int)t.p[k].dst && pc.sk == t.p[k].src,
              "item %u of %u (np %d): piece %d first %d len %d dst %d src %08x, want %d %u %d %d %08x", item, t.items, t.np, pc.k, pc.first_item, pc.lk,
              pc.dst_off, pc.sk, k, first, t.p[k].len, t.p[k].dst, t.p[k].src);
        if (pc.k != k) continue;
        const uint8_t* const base = (pc.sk & FMT_LIT_BIT) ? lit.data() : text.data();
        const int off = gen_window_off(pc.lk, (uint32_t)(uintptr_t)base, pc.sk, (int)item - pc.first_item);
        CHECK(off >= 0 && off + (pc.lk >= 16 ? 16 : pc.lk) <= pc.lk, "window outside its piece: lk %d off %d", pc.lk, off);
        copy_item(out + pc.dst_off, base + (pc.sk & ~FMT_LIT_BIT), pc.lk, off, &covered, pc.dst_off);
        ++items_seen;
    }
    // an item behind the record's last one is piece 0 (the kernel's lanes without work)
    if (t.items < 64) CHECK(plan_piece_of(pb, t.items).k == 0, "an idle lane's piece is not piece 0");
    for (int k = 0; k < t.np; ++k) {
        const uint8_t* const s = ((t.p[k].src & FMT_LIT_BIT) ? lit.data() : text.data()) + (t.p[k].src & ~FMT_LIT_BIT);
        CHECK(memcmp(out + t.p[k].dst, s, t.p[k].len) == 0, "piece %d of %d: bytes differ (len %d)", k, t.np, t.p[k].len);
    }
    for (uint32_t i = 0; i < t.total; ++i) CHECK(covered[i] > 0, "byte %u of a record of %u not written", i, t.total);
    free(out);
    return 1;
}

int main() {
    uint64_t pairs1 = 0, windows1 = 0;
    for (int len = 16; len <= 512; ++len)
        for (uint32_t align = 0; align < 16; ++align) { windows1 += whole_record(align, len); ++pairs1; }
    printf("fmtcopy| whole records: %llu (length, alignment) pairs, %llu windows\n", (unsigned long long)pairs1, (unsigned long long)windows1);

    uint64_t pairs2 = 0, windows2 = 0;
    for (int lk = 1; lk <= 1100; ++lk)
        for (uint32_t align = 0; align < 16; ++align) {
            windows2 += general_piece(align, lk, false);
            if (lk >= 16) ++pairs2;
            if (lk <= 64) general_piece(align, lk, true);       // literals: plain windows whatever their length
        }
    printf("fmtcopy| general pieces: %llu (length, alignment) pairs, %llu windows\n", (unsigned long long)pairs2, (unsigned long long)windows2);

    uint64_t plans = 0, inline_plans = 0, refused = 0, items_seen = 0;
    int refused_9 = 0, refused_65 = 0, refused_5 = 0, refused_short = 0, full_64 = 0, four_patches = 0;
    for (int it = 0; it < 40000; ++it) {
        const int np = 1 + (int)(rnd() % 8u);
        Made m = make_task(np, (int)(rnd() % 5u), false);
        if (m.t.n_patch == 4 && m.t.items <= 64) ++four_patches;
        if (m.t.items > 64) ++refused_65;
        if (m.t.items == 64) ++full_64;
        const int ok = one_plan(m, items_seen);
        ++plans; inline_plans += (uint64_t)ok; refused += (uint64_t)!ok;
    }
    // exactly 64 and 65 work items: 200-byte pieces are 14 items each, 16-byte pieces one
    for (int extra = 0; extra < 2; ++extra) {
        Made m = make_task(8, 0, false);
        const int lens[8] = {200, 200, 200, 200, 16, 16, 16, extra ? 47 : 31};      // 56 + 3 + (3 | 2) ... topped up below
        uint32_t o = 0, items = 0;
        for (int k = 0; k < 8; ++k) { m.t.p[k].len = (uint16_t)lens[k]; m.t.p[k].src = 64 + 300u * (uint32_t)k; m.t.p[k].dst = (uint16_t)o; o += (uint32_t)lens[k]; items += piece_items((uint32_t)lens[k]); }
        while (items < 64u + (uint32_t)extra) { m.t.p[7].len = (uint16_t)(m.t.p[7].len + 16); o += 16; items = 0; for (int k = 0; k < 8; ++k) items += piece_items(m.t.p[k].len); }
        m.t.total = (uint16_t)o; m.t.items = (uint16_t)items; m.text_bytes = 64 + 300 * 8 + 600;
        CHECK(items == 64u + (uint32_t)extra, "could not build a list of %u items: %u", 64u + (uint32_t)extra, items);
        const int ok = one_plan(m, items_seen);
        CHECK(ok == !extra, "%u work items: inline_ok %d", items, ok);
        ++plans; if (extra) ++refused_65; else ++full_64;
    }
    for (int it = 0; it < 200; ++it) {
        Made m9 = make_task(9 + it % 2, 0, false);
        CHECK(one_plan(m9, items_seen) == 0, "a list of %d pieces fits a plan", m9.t.np);
        ++refused_9; ++plans;
        Made m5 = make_task(1 + (int)(rnd() % 8u), 0, false);
        if (has_piece(m5.t, false) && m5.t.items <= 64) {
            Made m5b = m5;
            for (int e = 0; e < 5 + it % 2; ++e) {
                int k = 0;
                while (m5b.t.p[k].len < 16) ++k;
                m5b.t.patch[m5b.t.n_patch++] = ((uint32_t)m5b.t.p[k].dst + (uint32_t)e) | (65u << 16);
            }
            CHECK(one_plan(m5b, items_seen) == 0, "a list with %d patches fits a plan", m5b.t.n_patch);
            ++refused_5; ++plans;
        }
        Made ms = make_task(2 + (int)(rnd() % 7u), 1, true);
        if (ms.t.n_patch == 1 && ms.t.items <= 64) {
            CHECK(one_plan(ms, items_seen) == 0, "a patch inside a short piece fits a plan");
            ++refused_short; ++plans;
        }
    }
    printf("fmtcopy| plans: %llu lists, %llu inline (%llu work items decoded), refused: %d for pieces, %d for work items, %d for patches, %d for a patch in a short piece; "
           "%d of exactly 64 items, %d with four patches\n", (unsigned long long)plans, (unsigned long long)inline_plans, (unsigned long long)items_seen,
           refused_9, refused_65, refused_5, refused_short, full_64, four_patches);
    CHECK(refused_9 == 200 && refused_65 >= 1 && refused_5 >= 100 && refused_short >= 50 && full_64 >= 1 && four_patches >= 1000 && inline_plans >= 30000,
          "the plan cases are not all there");
    (void)refused;
    if (fails) { printf("%d fmtcopy checks FAILED\n", fails); return 1; }
    printf("all fmtcopy window and plan checks passed\n");
    return 0;
}
