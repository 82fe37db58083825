// csrc/aqc_revcopy.hpp on the CPU: the per-window functions of the merged-read pass (fmt_merged_kernel) — window count, source and
// destination offsets, the 16-byte reversal, the four-at-a-time complement — compiled without HIP and dealt out by a plain loop
// over the work items, the way the kernel's lanes take them.  For every (source offset mod 16, destination offset mod 16, p) with
// p = 0 .. 49 a piece of p bytes is copied reversed (plain, and complemented) and compared with a byte loop; the source and the
// destination live in heap blocks that END with the piece (a short piece's window ends with it and reads up to 16 bytes in front,
// which the program checks itself), so that any access behind is an ASan report.
// The complement is also checked against the table of comp_or_n for all 256 byte values in every position of a dword.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_revcopy.hpp"

using namespace aqc;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } } while (0)

static uint8_t comp_ref(uint8_t c) {
    switch (c) {
        case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
        case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
        case 'N': return 'N';
        default: return 'N';
    }
}

static RevWin load16(const uint8_t* p) { RevWin v; memcpy(&v, p, 16); return v; }

// the low n bytes of v (the kernel's 8 + 4 + 2 + 1 stores write exactly these)
static void store_low(uint8_t* d, const RevWin& v, uint32_t n) { memcpy(d, &v, n); }

static uint64_t run_piece(uint32_t so, uint32_t dof, uint32_t p, bool comp, uint32_t seed) {
    // source: a heap block that ends with the piece and puts it at an address = so (mod 16), 16 + so readable bytes in front of it (the
    // kernel may read 16: checked below); destination: a block that ends with the p bytes, at an address = dof (mod 16), canaries in front
    uint8_t* blk = (uint8_t*)malloc(so + 16 + p);
    uint8_t* dall = (uint8_t*)malloc(dof + p + 1) ;
    CHECK(((uintptr_t)blk & 15) == 0 && ((uintptr_t)dall & 15) == 0, "malloc is not 16-byte aligned");
    uint8_t* const piece = blk + so + 16;
    uint8_t* const dblk = dall + dof;
    const uint32_t a = (0u - (uint32_t)(uintptr_t)piece) & 15u;      // as the kernel derives it
    static const char alphabet[] = "ACGTacgtNnXx.-\n\0\x7f\xff";
    uint32_t x = seed * 2654435761u + 12345u;
    for (uint32_t i = 0; i < so + 16 + p; ++i) {
        x = x * 1664525u + 1013904223u;
        blk[i] = (uint8_t)alphabet[(x >> 24) % (sizeof(alphabet) - 1)];
    }
    const uint8_t* src = piece;
    memset(dall, 0xEE, dof + p + 1);
    std::vector<int> covered(p, 0);
    const uint32_t ni = revc_items(p, a);
    uint64_t windows = 0;
    for (uint32_t it = 0; it < ni; ++it) {
        const int off = revc_src_off(p, a, it);
        CHECK(off >= -16 && off + 16 <= (int)p, "source window outside: so %u p %u item %u off %d", so, p, it, off);
        CHECK(p < 16 || off >= 0, "negative offset of a long piece: p %u off %d", p, off);
        // every window but the first and the last of a long piece stands on the source's 16-byte grid
        if (p >= 16 && it > 0 && it + 1 < ni) CHECK(((so + (uint32_t)off) & 15u) == 0, "window off the grid: so %u p %u item %u off %d", so, p, it, off);
        RevWin v = revc_reverse(load16(src + off));
        if (comp) v = revc_comp16(v);
        const int d = revc_dst_off(p, off);
        CHECK(d >= 0 && (p < 16 ? d == 0 : d + 16 <= (int)p), "destination window outside: p %u off %d d %d", p, off, d);
        if (p >= 16) { memcpy(dblk + d, &v, 16); for (int i = 0; i < 16; ++i) covered[d + i]++; }
        else { store_low(dblk + d, v, p); for (uint32_t i = 0; i < p; ++i) covered[i]++; }
        ++windows;
    }
    for (uint32_t j = 0; j < p; ++j) {
        const uint8_t want = comp ? comp_ref(src[p - 1 - j]) : src[p - 1 - j];
        CHECK(covered[j] > 0, "byte %u of p %u not written (so %u)", j, p, so);
        CHECK(dblk[j] == want, "so %u do %u p %u comp %d byte %u: %02x, want %02x", so, dof, p, (int)comp, j, dblk[j], want);
    }
    CHECK(ni <= (p + 15) / 16 + 1, "too many windows: p %u a %u -> %u", p, a, ni);
    for (uint32_t i = 0; i < dof; ++i) CHECK(dall[i] == 0xEE, "byte in front of the destination written: so %u do %u p %u", so, dof, p);
    free(blk);
    free(dall);
    return windows;
}

int main() {
    // the complement of four bytes at once, every byte value in every position, with every kind of neighbour
    static const uint8_t neigh[] = {'A', 'n', 0x00, 0xff, 't', 0x20};
    for (uint32_t c = 0; c < 256; ++c)
        for (int pos = 0; pos < 4; ++pos)
            for (uint8_t nb : neigh) {
                uint32_t d = 0;
                for (int i = 0; i < 4; ++i) d |= (uint32_t)(i == pos ? c : nb) << (8 * i);
                const uint32_t r = revc_comp4(d);
                for (int i = 0; i < 4; ++i) {
                    const uint8_t in = (uint8_t)(d >> (8 * i)), got = (uint8_t)(r >> (8 * i));
                    CHECK(got == comp_ref(in), "comp4 %08x byte %d: %02x -> %02x, want %02x", d, i, in, got, comp_ref(in));
                }
            }
    // reversal
    {
        uint8_t b[16], o[16];
        for (int i = 0; i < 16; ++i) b[i] = (uint8_t)(i * 7 + 1);
        const RevWin r = revc_reverse(load16(b));
        memcpy(o, &r, 16);
        for (int i = 0; i < 16; ++i) CHECK(o[i] == b[15 - i], "reverse byte %d", i);
    }
    uint64_t windows = 0, pieces = 0;
    for (uint32_t so = 0; so < 16; ++so)
        for (uint32_t dof = 0; dof < 16; ++dof)
            for (uint32_t p = 0; p < 50; ++p)
                for (int comp = 0; comp < 2; ++comp) {
                    windows += run_piece(so, dof, p, comp != 0, so * 977u + dof * 131u + p * 7u + (uint32_t)comp);
                    ++pieces;
                }
    printf("revcopy| %llu pieces, %llu windows\n", (unsigned long long)pieces, (unsigned long long)windows);
    if (fails) { printf("%d revcopy checks FAILED\n", fails); return 1; }
    printf("all revcopy window checks passed\n");
    return 0;
}
