// adapter_selftest.cpp — the per-read functions of the adapter pass (afterqc_amd/csrc/aqc_adapter.hpp) without HIP: the lanes of a
// group are dealt out by plain loops, as adapter_cut_kernel deals them to the lanes of a wave, and the result is compared with
// vectors that tests/adapter_rule.py wrote.  argv[1]: the vector file, one case per line:
//   A <K> <adapter> <n> <2n hex digits | -> <p | -1>       a read and the place the model ends it at (-1: no match)
//   V <c0> <c1> <p | -1> <c0'> <c1'>                        the view that came in, the match, the view that goes out
//   M <8 hex digits> <left> <count>                         a dword of differences, the bytes still compared, how many are not zero
// Built plain and with -fsanitize=address,undefined by tests/test_adapter_rule.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_adapter.hpp"

using namespace aqc;

// one read through a group of G lanes.  `read` holds the n bytes and exactly the 15 bytes a lane's 16-byte load may take behind them.
template <int G>
static int group_first(const uint8_t* read, int n, const AdapterOpts& a) {
    constexpr int CAP = 16 * G;
    std::vector<uint32_t> row(CAP / 4 + ADP_ROW_TAIL, 0xA5A5A5A5u);
    for (int j = 0; j < ADP_ROW_TAIL; ++j) row[CAP / 4 + j] = 0u;        // (the kernel clears the words behind the row once)
    for (int g = 0; g < G; ++g) {
        const int nvalid = vp_nvalid(n, g);
        uint32_t d[4] = {0, 0, 0, 0};
        if (nvalid > 0) memcpy(d, read + 16 * g, 16);                    // (a whole 16-byte load: the padding is read)
        adp_keep16(d, nvalid);
        memcpy(row.data() + 4 * g, d, 16);
    }
    int p = ADP_NONE;
    for (int g = 0; g < G; ++g) p = vp_min(p, adp_lane_first<G>(row.data(), n, a.w[0], a.len[0], a.min_overlap, g));
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: adapter_selftest <vectors>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static char buf[8192], hex[4096], adapter[128];
    long searches = 0, views = 0, words = 0, failed = 0;
    while (fgets(buf, sizeof(buf), f)) {
        if (buf[0] == 'A') {
            AdapterOpts a{};
            int n = 0, want = 0;
            if (sscanf(buf, "A %d %100s %d %4095s %d", &a.min_overlap, adapter, &n, hex, &want) != 5) { fprintf(stderr, "bad line: %s", buf); return 2; }
            a.len[0] = (int)strlen(adapter);
            if (!adp_opts_ok(a)) { fprintf(stderr, "options out of range: %s", buf); return 2; }
            memcpy(a.w[0], adapter, (size_t)a.len[0]);
            uint8_t* const read = (uint8_t*)malloc((size_t)n + 15);      // anything further is out of bounds
            memset(read, 0xAA, (size_t)n + 15);
            for (int i = 0; i < n; ++i) {
                unsigned v = 0;
                sscanf(hex + 2 * i, "%2x", &v);
                read[i] = (uint8_t)v;
            }
            for (int G : {8, 16, 32, 64}) {
                if (n > 16 * G) continue;
                const int p = G == 8 ? group_first<8>(read, n, a) : G == 16 ? group_first<16>(read, n, a) : G == 32 ? group_first<32>(read, n, a) : group_first<64>(read, n, a);
                ++searches;
                if ((p == ADP_NONE ? -1 : p) != want) {
                    if (++failed <= 20) printf("FAIL G=%d: %.70s ... got %d want %d\n", G, buf, p == ADP_NONE ? -1 : p, want);
                }
            }
            free(read);
        } else if (buf[0] == 'V') {
            int c0, c1, p, o0, o1;
            if (sscanf(buf, "V %d %d %d %d %d", &c0, &c1, &p, &o0, &o1) != 5) { fprintf(stderr, "bad line: %s", buf); return 2; }
            const uint32_t v = view_end(view_word(c0, c1), p >= 0, p);
            ++views;
            if (view_c0(v) != o0 || view_c1(v) != o1) {
                if (++failed <= 20) printf("FAIL view: %s got %d %d\n", buf, view_c0(v), view_c1(v));
            }
        } else if (buf[0] == 'M') {
            unsigned x;
            int left, want;
            if (sscanf(buf, "M %x %d %d", &x, &left, &want) != 3) { fprintf(stderr, "bad line: %s", buf); return 2; }
            const int got = adp_mismatch4((uint32_t)x & adp_tail_mask(left));
            ++words;
            if (got != want) {
                if (++failed <= 20) printf("FAIL word: %s got %d\n", buf, got);
            }
        }
    }
    fclose(f);
    printf("%ld searches, %ld views, %ld words checked\n", searches, views, words);
    if (failed) { printf("%ld FAILED\n", failed); return 1; }
    printf("all adapter checks passed\n");
    return 0;
}
