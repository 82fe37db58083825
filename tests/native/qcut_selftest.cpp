// qcut_selftest.cpp — the per-read functions of the quality cut (afterqc_amd/csrc/aqc_qcut.hpp) without HIP: the lanes of a group are
// dealt out by plain loops, exactly as quality_cut_kernel deals them to the lanes of a wave, and the result is compared with vectors
// that tests/cut_rule.py wrote.  argv[1]: the vector file, one case per line:
//   W <window> <mean quality> <front> <tail> <right> <n> <2n hex digits | -> <c0> <c1>      a line and the view the model gives
//   S <len> <trim front> <trim tail> <c0> <c1> <start> <length>                              trim() and [c0:c1] of a string of len bytes
// Built plain and with -fsanitize=address,undefined by tests/test_cut_rule.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_qcut.hpp"

using namespace aqc;

// one read through a group of G lanes; the line is followed by `pad` readable bytes, as an arena is
static uint32_t group_view(const std::vector<uint8_t>& line, int n, const QcutOpts& o, int G) {
    std::vector<int> area(16 * G + 4, 0);
    int* const P = area.data() + 3;
    P[0] = 0;
    // 16 bytes per lane, their running sums, the scan of the lane totals
    std::vector<int> total(G, 0);
    std::vector<std::vector<int>> p(G, std::vector<int>(16, 0));
    for (int g = 0; g < G; ++g) {
        const int nvalid = vp_nvalid(n, g);
        uint32_t d[4] = {0, 0, 0, 0};
        if (nvalid > 0) memcpy(d, line.data() + 16 * g, 16);          // (a whole 16-byte load: the padding is read)
        qcut_sum16(d[0], d[1], d[2], d[3], nvalid, p[g].data());
        total[g] = p[g][15];
    }
    int base = 0;
    for (int g = 0; g < G; ++g) {
        for (int k = 0; k < 16; ++k) area[4 + 16 * g + k] = base + p[g][k];
        base += total[g];
    }
    const int w = qcut_window(o, n), thr = o.mean_quality * w;
    const int starts = n > 0 ? n - w + 1 : 0;
    const int passes = (starts + G - 1) / G;
    std::vector<uint32_t> bits(G);
    for (int g = 0; g < G; ++g) bits[g] = qcut_lane_bits(P, n, w, thr, g, G, passes);
    int first_good = QCUT_NONE, last_good = -1;
    for (int g = 0; g < G; ++g) {
        first_good = vp_min(first_good, qcut_lane_first(bits[g] >> 16, g, G, 0));
        last_good = vp_max(last_good, qcut_lane_last(bits[g] >> 16, g, G));
    }
    const int c0 = first_good == QCUT_NONE ? 0 : qcut_front(o, first_good);
    int first_bad = QCUT_NONE;
    for (int g = 0; g < G; ++g) first_bad = vp_min(first_bad, qcut_lane_first((bits[g] & 0xffffu) & ~(bits[g] >> 16), g, G, c0));
    return qcut_view(o, n, w, first_good, last_good, first_bad);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: qcut_selftest <vectors>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static char buf[8192];
    long windows = 0, slices = 0, failed = 0;
    while (fgets(buf, sizeof(buf), f)) {
        if (buf[0] == 'W') {
            QcutOpts o{};
            int n = 0, c0 = 0, c1 = 0;
            static char hex[4096];
            if (sscanf(buf, "W %d %d %d %d %d %d %4095s %d %d", &o.window, &o.mean_quality, &o.front, &o.tail, &o.right, &n, hex, &c0, &c1) != 9) { fprintf(stderr, "bad line: %s", buf); return 2; }
            if (!qcut_opts_ok(o)) { fprintf(stderr, "options out of range: %s", buf); return 2; }
            // the line exactly as long as it is plus the 15 bytes a lane's load may take behind it: anything further is out of bounds
            std::vector<uint8_t> line((size_t)n + 15, 0xAA);
            for (int i = 0; i < n; ++i) {
                unsigned v = 0;
                sscanf(hex + 2 * i, "%2x", &v);
                line[i] = (uint8_t)v;
            }
            for (int G : {8, 16, 32, 64}) {
                if (n > 16 * G) continue;
                const uint32_t view = group_view(line, n, o, G);
                ++windows;
                if (view_c0(view) != c0 || view_c1(view) != c1) {
                    if (++failed <= 20) printf("FAIL G=%d: %.60s ... got %d %d want %d %d\n", G, buf, view_c0(view), view_c1(view), c0, c1);
                }
            }
        } else if (buf[0] == 'S') {
            int len, tf, tt, c0, c1, st, nl;
            if (sscanf(buf, "S %d %d %d %d %d %d %d", &len, &tf, &tt, &c0, &c1, &st, &nl) != 7) { fprintf(stderr, "bad line: %s", buf); return 2; }
            int a = 7, l = len;                     // (a view that already starts 7 bytes in: the function moves it)
            view_apply(a, l, tf, tt, view_word(c0, c1));
            ++slices;
            if (l != nl || (nl > 0 && a != 7 + st)) {
                if (++failed <= 20) printf("FAIL slice: %s got %d %d\n", buf, a - 7, l);
            }
        }
    }
    fclose(f);
    printf("%ld group views, %ld slices checked\n", windows, slices);
    if (failed) { printf("%ld FAILED\n", failed); return 1; }
    printf("all quality cut checks passed\n");
    return 0;
}
