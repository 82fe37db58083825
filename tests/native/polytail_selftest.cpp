// polytail_selftest.cpp — the per-read functions of the poly-tail pass (afterqc_amd/csrc/aqc_polytail.hpp) without HIP: the lanes of
// a group are dealt out by plain loops, as poly_tail_kernel deals them to the lanes of a wave, and the result is compared with
// vectors that tests/poly_rule.py wrote.  argv[1]: the vector file, one case per line:
//   P <La> <Lc> <Lg> <Lt> <n> <2n hex digits | -> <end>     a read, the four minimum lengths (0: off) and where the model ends it
//   V <c0> <c1> <n> <end> <c0'> <c1'>                        the view that came in, the line's length and end, the view that goes out
//   M <32 hex digits> <letter> <nvalid> <mask>               a lane's 16 bytes, and which of the first nvalid are not the letter
// Built plain and with -fsanitize=address,undefined by tests/test_poly_rule.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_polytail.hpp"

using namespace aqc;

// one read through a group of G lanes.  `read` holds the n bytes and exactly the 15 bytes a lane's 16-byte load may take behind them.
template <int G>
static int group_end(const uint8_t* read, int n, const PolyOpts& o) {
    int end = n;
    for (int x = 0; x < POLY_LETTERS; ++x) {
        const int L = o.min_len[x];
        if (L == 0) continue;
        uint32_t mm[G], valid[G];
        for (int g = 0; g < G; ++g) {
            const int nvalid = vp_nvalid(n, g);
            uint32_t d[4] = {0, 0, 0, 0};
            if (nvalid > 0) memcpy(d, read + 16 * g, 16);                // (a whole 16-byte load: the padding is read)
            mm[g] = poly_mismatch16(d, poly_letter(x), nvalid);
            valid[g] = poly_valid16(nvalid);
        }
        int mm_w = 0;                                                    // (the kernel: the last byte's lane and its neighbour)
        for (int g = 0; g < G; ++g) mm_w += poly_window_count(mm[g], n, g, poly_window(L));
        if (!poly_candidate(n, L, mm_w)) continue;                       // the test in front of the scan: the letter cannot pass
        int first_fail = POLY_NONE, behind = 0;
        for (int g = G - 1; g >= 0; --g) {                               // (the kernel: a wave-wide prefix sum, the group's last minus the lane's)
            first_fail = vp_min(first_fail, poly_lane_fail(mm[g], behind, n, g, L));
            behind += poly_popc(mm[g]);
        }
        const int scanned = poly_scanned(first_fail, n);
        int t = 0;
        if (scanned >= L)
            for (int g = 0; g < G; ++g) t = vp_max(t, poly_lane_last(~mm[g] & valid[g], n, g, scanned));
        end = vp_min(end, poly_end(n, L, scanned, t));
    }
    return end;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: polytail_selftest <vectors>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static char buf[8192], hex[4096];
    long reads = 0, views = 0, masks = 0, failed = 0;
    while (fgets(buf, sizeof(buf), f)) {
        if (buf[0] == 'P') {
            PolyOpts o{};
            int n = 0, want = 0;
            if (sscanf(buf, "P %d %d %d %d %d %4095s %d", &o.min_len[0], &o.min_len[1], &o.min_len[2], &o.min_len[3], &n, hex, &want) != 7) { fprintf(stderr, "bad line: %s", buf); return 2; }
            if (!poly_opts_ok(o) || !poly_on(o)) { fprintf(stderr, "options out of range: %s", buf); return 2; }
            uint8_t* const read = (uint8_t*)malloc((size_t)n + 15);      // anything further is out of bounds
            memset(read, 'G', (size_t)n + 15);                           // (the padding looks like a tail: it must not count)
            for (int i = 0; i < n; ++i) {
                unsigned v = 0;
                sscanf(hex + 2 * i, "%2x", &v);
                read[i] = (uint8_t)v;
            }
            for (int G : {8, 16, 32, 64}) {
                if (n > 16 * G) continue;
                const int e = G == 8 ? group_end<8>(read, n, o) : G == 16 ? group_end<16>(read, n, o) : G == 32 ? group_end<32>(read, n, o) : group_end<64>(read, n, o);
                ++reads;
                if (e != want) {
                    if (++failed <= 20) printf("FAIL G=%d: %.70s ... got %d want %d\n", G, buf, e, want);
                }
            }
            free(read);
        } else if (buf[0] == 'V') {
            int c0, c1, n, end, o0, o1;
            if (sscanf(buf, "V %d %d %d %d %d %d", &c0, &c1, &n, &end, &o0, &o1) != 6) { fprintf(stderr, "bad line: %s", buf); return 2; }
            const uint32_t v = view_end(view_word(c0, c1), end < n, end);
            ++views;
            if (view_c0(v) != o0 || view_c1(v) != o1) {
                if (++failed <= 20) printf("FAIL view: %s got %d %d\n", buf, view_c0(v), view_c1(v));
            }
        } else if (buf[0] == 'M') {
            char letter;
            int nvalid;
            unsigned want;
            if (sscanf(buf, "M %32s %c %d %x", hex, &letter, &nvalid, &want) != 4) { fprintf(stderr, "bad line: %s", buf); return 2; }
            uint8_t b[16];
            for (int i = 0; i < 16; ++i) {
                unsigned v = 0;
                sscanf(hex + 2 * i, "%2x", &v);
                b[i] = (uint8_t)v;
            }
            uint32_t d[4];
            memcpy(d, b, 16);
            const uint32_t got = poly_mismatch16(d, (uint8_t)letter, nvalid);
            ++masks;
            if (got != want) {
                if (++failed <= 20) printf("FAIL mask: %s got %x\n", buf, got);
            }
        }
    }
    fclose(f);
    printf("%ld reads, %ld views, %ld masks checked\n", reads, views, masks);
    if (failed) { printf("%ld FAILED\n", failed); return 1; }
    printf("all poly-tail checks passed\n");
    return 0;
}
