// csrc/aqc_gzlz.hpp on the CPU: the functions a lane of gz_encode_lz_kernel / gz_hist_lz_kernel runs — hash, insert, chain walk
// with extension, token decision — compiled without HIP and dealt out by plain loops in the kernel's order: a window of 64
// positions is inserted whole, then searched, then parsed greedily.  argv: files; each is cut into members of 0xff00 bytes as a
// stream is, and for every level 6 .. 9 every token of every member is checked (length, distance, bytes, tiling), the members
// are encoded with the code aqcgz::build_codebook makes of the sampling pass's counts, and zlib inflates each one on its own.
// Every member lives in a heap block of exactly its size: a load past text + n is an ASan report.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_gz.hpp"
#include "../../afterqc_amd/csrc/aqc_gzlz.hpp"

using namespace aqc;

constexpr int MEMBER = 0xff00;

struct Tok {
    int pos, len, dist;      // len 1: a literal
};

template <bool EXACT>
static void tokenize(const uint8_t* s, int n, int depth, const uint32_t* lc, const uint32_t* dc, std::vector<Tok>& out) {
    std::vector<uint16_t> head(1 << GZLZ_HASH_BITS, (uint16_t)GZLZ_NIL), prev(GZLZ_PREV, (uint16_t)GZLZ_NIL);
    const int n_win = (n + GZLZ_WINDOW - 1) / GZLZ_WINDOW;
    int skip = 0;
    for (int w = 0; w < n_win; ++w) {
        for (int lane = 0; lane < GZLZ_WINDOW; ++lane) {
            const int p = GZLZ_WINDOW * w + lane;
            if (p + 2 < n) gzlz_link(head.data(), prev.data(), p, gzlz_hash(s, p));
        }
        if (skip >= GZLZ_WINDOW) { skip -= GZLZ_WINDOW; continue; }
        int blen[GZLZ_WINDOW], dist[GZLZ_WINDOW];
        for (int lane = 0; lane < GZLZ_WINDOW; ++lane) {
            const int p = GZLZ_WINDOW * w + lane;
            blen[lane] = 1; dist[lane] = 0;
            if (p < n && lane >= skip) {
                const GzlzMatch m = gzlz_search(s, n, p, prev.data(), depth);
                if (gzlz_take<EXACT>(s, p, m, lc, dc)) { blen[lane] = m.len; dist[lane] = m.dist; }
            }
        }
        const int end = n - GZLZ_WINDOW * w < GZLZ_WINDOW ? n - GZLZ_WINDOW * w : GZLZ_WINDOW;
        int e = skip;
        while (e < end) {
            out.push_back({GZLZ_WINDOW * w + e, blen[e], dist[e]});
            e += blen[e];
        }
        if (e < GZLZ_WINDOW) e = GZLZ_WINDOW;
        skip = e - GZLZ_WINDOW;
    }
}

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } } while (0)

static void check_tokens(const char* name, int level, int member, const uint8_t* s, int n, const std::vector<Tok>& t) {
    int at = 0;
    for (const Tok& k : t) {
        CHECK(k.pos == at, "%s level %d member %d: token at %d, %d expected", name, level, member, k.pos, at);
        if (k.len == 1) { at += 1; continue; }
        CHECK(k.len >= 3 && k.len <= 258, "%s level %d member %d pos %d: length %d", name, level, member, k.pos, k.len);
        CHECK(k.dist >= 1 && k.dist <= 32768 && k.dist <= k.pos, "%s level %d member %d pos %d: distance %d", name, level, member, k.pos, k.dist);
        CHECK(k.pos + k.len <= n, "%s level %d member %d pos %d: length %d runs past %d", name, level, member, k.pos, k.len, n);
        if (k.dist >= 1 && k.dist <= k.pos && k.pos + k.len <= n)
            CHECK(memcmp(s + k.pos, s + k.pos - k.dist, (size_t)k.len) == 0, "%s level %d member %d pos %d: the copy differs", name, level, member, k.pos);
        at += k.len;
    }
    CHECK(at == n, "%s level %d member %d: tokens cover %d of %d bytes", name, level, member, at, n);
}

struct Bits {
    std::vector<uint8_t> out;
    unsigned long long acc = 0;
    int nacc = 0;
    void put(uint32_t v, int len) {
        acc |= (unsigned long long)v << nacc;
        nacc += len;
        while (nacc >= 8) { out.push_back((uint8_t)acc); acc >>= 8; nacc -= 8; }
    }
    void finish() { if (nacc) { out.push_back((uint8_t)acc); acc = 0; nacc = 0; } }
};

static void encode(const aqcgz::GzCodebook& cb, const uint8_t* s, const std::vector<Tok>& t, Bits& b) {
    for (uint32_t i = 0; i < cb.hdr_bits; i += 32) {
        const int k = cb.hdr_bits - i < 32 ? (int)(cb.hdr_bits - i) : 32;
        const uint32_t v = cb.hdr[i / 32];
        b.put(v & 0xffffu, k < 16 ? k : 16);
        if (k > 16) b.put((v >> 16) & ((1u << (k - 16)) - 1u), k - 16);
    }
    for (const Tok& k : t) {
        if (k.len == 1) { b.put(cb.lit[s[k.pos]] & 0xffffu, (int)(cb.lit[s[k.pos]] >> 16)); continue; }
        const int ls = len_sym(k.len), ds = dist_sym(k.dist);
        b.put(cb.lit[257 + ls] & 0xffffu, (int)(cb.lit[257 + ls] >> 16));
        b.put((uint32_t)(k.len - len_base(ls)), len_extra(ls));
        b.put(cb.dist[ds] & 0xffffu, (int)(cb.dist[ds] >> 16));
        b.put((uint32_t)(k.dist - dist_base(ds)), dist_extra(ds));
    }
    b.put(cb.lit[256] & 0xffffu, (int)(cb.lit[256] >> 16));
    b.finish();
}

static bool inflates_to(const std::vector<uint8_t>& raw, const uint8_t* s, int n) {
    std::vector<uint8_t> back((size_t)n + 16);
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) return false;
    z.next_in = const_cast<uint8_t*>(raw.data()); z.avail_in = (uInt)raw.size();
    z.next_out = back.data(); z.avail_out = (uInt)back.size();
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.total_out == (uLong)n && z.avail_in == 0 && (n == 0 || memcmp(back.data(), s, (size_t)n) == 0);
    inflateEnd(&z);
    return ok;
}

int main(int argc, char** argv) {
    int checks = 0;
    // the closed forms against RFC 1951's tables, every length and distance
    for (int len = 3; len <= 258; ++len) {
        const int ls = len_sym(len);
        CHECK(ls >= 0 && ls < 29 && len >= len_base(ls) && len - len_base(ls) < (1 << len_extra(ls)), "length %d -> symbol %d", len, ls);
    }
    for (int d = 1; d <= 32768; ++d) {
        const int ds = dist_sym(d);
        CHECK(ds >= 0 && ds < 30 && d >= dist_base(ds) && d - dist_base(ds) < (1 << dist_extra(ds)), "distance %d -> symbol %d", d, ds);
    }
    int last_depth = 0;
    for (int level = 6; level <= 9; ++level) {
        CHECK(gzlz_depth(level) > last_depth && gzlz_depth(level) <= 64, "depth of level %d", level);
        last_depth = gzlz_depth(level);
    }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> data;
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + got);
        fclose(f);
        // every member in a block of its own, exactly its size
        std::vector<std::vector<uint8_t>> members;
        for (size_t o = 0; o < data.size(); o += MEMBER) members.emplace_back(data.begin() + o, data.begin() + std::min(data.size(), o + MEMBER));
        size_t sizes[4] = {0, 0, 0, 0};
        for (int level = 6; level <= 9; ++level) {
            const int depth = gzlz_depth(level);
            uint32_t hist[320];
            memset(hist, 0, sizeof(hist));
            for (size_t k = 0; k < members.size() && k < 16; ++k) {
                std::vector<Tok> t;
                tokenize<false>(members[k].data(), (int)members[k].size(), depth, nullptr, nullptr, t);
                check_tokens(argv[a], level, (int)k, members[k].data(), (int)members[k].size(), t);
                for (const Tok& x : t) {
                    if (x.len == 1) hist[members[k][x.pos]]++;
                    else { hist[257 + len_sym(x.len)]++; hist[286 + dist_sym(x.dist)]++; }
                }
            }
            aqcgz::GzCodebook cb;
            if (!aqcgz::build_codebook(hist, hist + 286, &cb)) { printf("FAIL %s level %d: no code\n", argv[a], level); return 1; }
            for (size_t k = 0; k < members.size(); ++k) {
                const uint8_t* s = members[k].data();
                const int n = (int)members[k].size();
                std::vector<Tok> t;
                tokenize<true>(s, n, depth, cb.lit, cb.dist, t);
                check_tokens(argv[a], level, (int)k, s, n, t);
                Bits b;
                encode(cb, s, t, b);
                CHECK(inflates_to(b.out, s, n), "%s level %d member %zu: zlib does not inflate it to its text", argv[a], level, k);
                sizes[level - 6] += std::min(b.out.size(), (size_t)n + 5) + 26;
            }
        }
        printf("gzlz| %-40s text %8zu  level 6 %8zu  7 %8zu  8 %8zu  9 %8zu\n", argv[a], data.size(), sizes[0], sizes[1], sizes[2], sizes[3]);
        ++checks;
    }
    if (fails) { printf("%d gzlz checks FAILED\n", fails); return 1; }
    printf("all %d gzlz logic checks passed\n", checks);
    return 0;
}
