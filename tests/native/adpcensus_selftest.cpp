// adpcensus_selftest.cpp — the per-read functions of the adapter census (afterqc_amd/csrc/aqc_adpcensus.hpp) without HIP: the lanes of
// a group are dealt out by plain loops, as adapter_census_kernel deals them to the lanes of a wave, and the result is compared with
// vectors that tests/detect_rule.py wrote.  argv[1]: the vector file, one case per line:
//   P <k> <probe> ... <probe>                   the k probes (12 letters each) of the reads that follow
//   R <n> <2n hex digits | -> <mask>            a read and the probes the model says it holds, bit i for probe i
//   B <k> <probe> ... <probe>                   a probe set cen_from_letters must refuse (a bad number, a letter that is no base)
// Built plain and with -fsanitize=address,undefined by tests/test_detect_rule.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_adpcensus.hpp"

using namespace aqc;

// one read through a group of G lanes.  `read` holds the n bytes and exactly the 15 bytes a lane's 16-byte load may take behind them.
template <int G>
static uint32_t group_held(const uint8_t* read, int n, const CensusProbes& P) {
    constexpr int CAP = 16 * G;
    std::vector<uint32_t> row(CAP / 4 + CEN_ROW_TAIL, 0xA5A5A5A5u);      // (exactly the kernel's row: anything further is out of bounds)
    for (int j = 0; j < CEN_ROW_TAIL; ++j) row[CAP / 4 + j] = 0u;        // (the kernel clears the words behind the row once)
    for (int g = 0; g < G; ++g) {
        const int nvalid = vp_nvalid(n, g);
        uint32_t d[4] = {0, 0, 0, 0};
        if (nvalid > 0) memcpy(d, read + 16 * g, 16);                    // (a whole 16-byte load: the padding is read)
        adp_keep16(d, nvalid);
        memcpy(row.data() + 4 * g, d, 16);
    }
    uint32_t held = 0;
    for (int g = 0; g < G; ++g) held |= cen_lane_held(row.data(), P, g);
    return held;
}

static bool parse_probes(char* line, CensusProbes& P) {
    static uint8_t seq[64][CEN_PROBE_LEN];
    memset(seq, 0, sizeof(seq));
    char* tok = strtok(line + 1, " \n");
    if (!tok) { fprintf(stderr, "bad probe line\n"); exit(2); }
    const int k = atoi(tok);
    int got = 0;
    while ((tok = strtok(nullptr, " \n")) && got < 64) {
        if (strlen(tok) != CEN_PROBE_LEN) { fprintf(stderr, "a probe of %zu letters\n", strlen(tok)); exit(2); }
        memcpy(seq[got++], tok, CEN_PROBE_LEN);
    }
    if (got != (k < 0 ? 0 : k > 64 ? 64 : k)) { fprintf(stderr, "probe line: %d announced, %d given\n", k, got); exit(2); }
    return cen_from_letters(k, seq, P);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: adpcensus_selftest <vectors>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static char buf[8192], hex[4096];
    long reads = 0, groups = 0, sets = 0, refused = 0, failed = 0;
    CensusProbes P{};
    while (fgets(buf, sizeof(buf), f)) {
        if (buf[0] == 'P') {
            if (!parse_probes(buf, P)) { fprintf(stderr, "probes refused\n"); return 2; }
            ++sets;
        } else if (buf[0] == 'B') {
            CensusProbes bad{};
            if (parse_probes(buf, bad)) {
                if (++failed <= 20) printf("FAIL: a bad probe set was taken\n");
            }
            ++refused;
        } else if (buf[0] == 'R') {
            int n = 0;
            unsigned want = 0;
            if (sscanf(buf, "R %d %4095s %u", &n, hex, &want) != 3) { fprintf(stderr, "bad line: %s", buf); return 2; }
            uint8_t* const read = (uint8_t*)malloc((size_t)n + 15);      // anything further is out of bounds
            memset(read, 0xAA, (size_t)n + 15);
            for (int i = 0; i < n; ++i) {
                unsigned v = 0;
                sscanf(hex + 2 * i, "%2x", &v);
                read[i] = (uint8_t)v;
            }
            ++reads;
            for (int G : {8, 16, 32, 64}) {
                if (n > 16 * G) continue;
                const uint32_t got = G == 8 ? group_held<8>(read, n, P) : G == 16 ? group_held<16>(read, n, P) : G == 32 ? group_held<32>(read, n, P) : group_held<64>(read, n, P);
                ++groups;
                if (got != want) {
                    if (++failed <= 20) printf("FAIL G=%d: %.70s ... got %u want %u\n", G, buf, got, want);
                }
            }
            free(read);
        }
    }
    fclose(f);
    printf("%ld probe sets, %ld reads, %ld groups, %ld refusals checked\n", sets, reads, groups, refused);
    if (failed) { printf("%ld FAILED\n", failed); return 1; }
    printf("all census checks passed\n");
    return 0;
}
