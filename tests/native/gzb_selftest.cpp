// gzb_selftest.cpp — the device gunzip's per-lane logic (afterqc_amd/csrc/aqc_gunzip_dev.hpp), run on the CPU.
//
// The header's GZB_HD functions are what the kernels' lanes execute: the block-start tests, the table builder, the block
// decoder, the chain walk, the marker re-basing.  CpuOffload (csrc/aqc_gunzip_ref.hpp) deals them out with plain loops in the kernels' order
// (scan -> compact -> decode -> chain -> gather, same buffers, same GzbJob) and plugs into the real ParallelGunzip through
// the SectionOffload interface the GPU uses (aqc_gunzip_offload.hip: DeviceInflate).  So this checks, without a GPU:
//   * every zlib stream below comes out byte-identical (ParallelGunzip also verifies CRC-32 / ISIZE itself);
//   * the offloaded sections really are committed (the chain rule accepts them) for dynamic-Huffman streams;
//   * stored blocks inside a chain, concatenated members, fixed-Huffman and stored-only streams, false section starts,
//     tiny symbol space (overflow -> host) and tiny candidate space all degrade to host decoding, never to wrong bytes.
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <memory>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_gunzip_dev.hpp"
#include "../../afterqc_amd/csrc/aqc_gunzip_ref.hpp"
#include "../../afterqc_amd/csrc/aqc_gz.hpp"

using namespace aqc;

namespace {

std::vector<uint8_t> fastq_like(size_t n_reads, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<uint8_t> t;
    const char B[] = "ACGT", Q[] = "#/6<AEEEEEEEEE";
    for (size_t r = 0; r < n_reads; ++r) {
        char name[96];
        const int nl = snprintf(name, sizeof(name), "@SIM:1:FC1:%u:%u:%u:%u 1:N:0:ACGT\n", (unsigned)(1 + rng() % 4), (unsigned)(1101 + rng() % 1200), (unsigned)(1000 + rng() % 24000), (unsigned)(1000 + rng() % 19000));
        t.insert(t.end(), name, name + nl);
        for (int i = 0; i < 150; ++i) t.push_back((uint8_t)(rng() % 500 == 0 ? 'N' : B[rng() & 3]));
        t.push_back('\n'); t.push_back('+'); t.push_back('\n');
        uint8_t q = 'E';
        for (int i = 0; i < 150; ++i) { if (rng() % 7 == 0) q = (uint8_t)Q[rng() % 14]; t.push_back(q); }
        t.push_back('\n');
    }
    return t;
}

std::vector<uint8_t> gz_of(const std::vector<uint8_t>& text, int level, int strategy, size_t flush_every = 0, int flush = Z_FULL_FLUSH) {
    z_stream zs{};
    deflateInit2(&zs, level, Z_DEFLATED, 15 + 16, 8, strategy);
    std::vector<uint8_t> out(deflateBound(&zs, (uLong)text.size()) + (flush_every ? text.size() / flush_every * 16 + 64 : 0) + 64);
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    size_t pos = 0;
    while (pos < text.size()) {
        const size_t k = flush_every ? std::min(flush_every, text.size() - pos) : text.size() - pos;
        zs.next_in = (Bytef*)text.data() + pos; zs.avail_in = (uInt)k;
        deflate(&zs, pos + k == text.size() ? Z_FINISH : flush);
        pos += k;
    }
    if (text.empty()) deflate(&zs, Z_FINISH);
    out.resize(zs.total_out);
    deflateEnd(&zs);
    return out;
}

int failures = 0;
uint32_t g_max_slices = 1u << 20, g_slice_tokens = 300;      // (a case may cut the decoder off: unfinished blocks then go to the host)

// decode gz through ParallelGunzip with the CPU emulation of the device as its offloader; returns the offloader's counters
long g_break_after = -1, g_resolve_breaks_after = -1;
bool g_resident = false;
int g_case_no = 0;
uint64_t g_segment_bytes = 0;
uint32_t g_tok_ratio = 8;
uint64_t g_sections_resolved = 0;
bool run_case(const char* what, const std::vector<uint8_t>& gz, const std::vector<uint8_t>& text, size_t section, size_t group, int threads, bool want_device,
              uint32_t ratio_cap = 20, uint32_t cand_div = 4096, bool expect_fail = false, bool hybrid = false) {
    CpuOffload off(group);
    ++g_case_no;
    off.break_after = g_break_after;
    off.resident = g_resident;
    off.resolve_breaks_after = g_resolve_breaks_after;
    off.tok_ratio = g_tok_ratio;
    off.overlap_tokens = g_tok_ratio <= 2 ? GZB_OVERLAP_TOKENS : 2048u;       // (the product's lean budget in file mode)
    off.ratio_cap = ratio_cap; off.cand_div = cand_div; off.max_slices = g_max_slices; off.slice_tokens = g_slice_tokens;
    aqc_host::Pool pool(threads);
    std::vector<uint8_t> out(text.size() + 65536);
    size_t produced = 0;
    bool failed = false;
    uint64_t dev_acc = 0, host_acc = 0, bridged = 0, res_bytes = 0, off_bytes = 0;
    {
        aqcgz::ParallelGunzip pg(gz.data(), gz.size(), threads ? &pool : nullptr, 4, section, &off, !hybrid);
        for (;;) {
            // resident mode, every other case: the text of resolved sections is LISTED, not copied (what the pipe's reader asks for);
            // the "device memory" of the emulation is host memory, so the check copies it into place itself — and counts the line
            // feeds of every whole piece against what resolve() reported
            std::vector<aqcgz::DevSegment> segs;
            const bool want_segs = g_resident && (g_case_no & 1);
            const size_t got = pg.read(out.data() + produced, std::min<size_t>(out.size() - produced, 777777), want_segs ? &segs : nullptr);
            if (pg.failed()) { failed = true; break; }
            if (!got) break;
            size_t last_end = 0;
            for (const aqcgz::DevSegment& g : segs) {
                if (g.dst_off < last_end || g.dst_off + g.len > got || g.sec_off + g.len > g.sec_len || !g.keep) { printf("bad device segment\n"); failed = true; break; }
                last_end = g.dst_off + g.len;
                memcpy(out.data() + produced + g.dst_off, g.dev, g.len);
                g_segment_bytes += g.len;
                const size_t pieces = (g.sec_len + aqcgz::NL_PIECE - 1) / aqcgz::NL_PIECE;
                for (size_t j = 0; j < pieces; ++j) {
                    const size_t hi = g.sec_len - (pieces - 1 - j) * aqcgz::NL_PIECE, lo = hi > aqcgz::NL_PIECE ? hi - aqcgz::NL_PIECE : 0;
                    if (lo < g.sec_off || hi > g.sec_off + g.len) continue;
                    const uint8_t* p = g.dev - g.sec_off + lo;
                    uint32_t c = 0;
                    for (size_t i = 0; i < hi - lo; ++i) c += p[i] == '\n';
                    if (c != g.piece_nl[j]) { printf("line feeds of piece %zu: %u counted, %u reported\n", j, c, g.piece_nl[j]); failed = true; }
                }
            }
            if (failed) break;
            produced += got;
        }
        dev_acc = pg.offloaded_accepted; host_acc = pg.sections_accepted - pg.offloaded_accepted; bridged = pg.bridged_bytes;
        res_bytes = pg.resident_bytes; off_bytes = pg.offloaded_bytes;
    }
    g_sections_resolved += off.sections_resolved;
    bool ok;
    if (expect_fail) ok = failed;
    else {
        ok = !failed && produced == text.size() && (text.empty() || memcmp(out.data(), text.data(), text.size()) == 0);
        if (ok && want_device && dev_acc == 0) ok = false;
        if (ok && hybrid && want_device && host_acc == 0) ok = false;      // the pool and the device both supplied sections
        if (ok && g_resident && res_bytes != off_bytes) ok = false;        // resident mode: no device section went through the host's translation
    }
    printf("%-46s %s  gz %8zu -> %9zu B  sec %7zu  device sections %3llu  host %3llu  bridged %9llu B  candidates %llu  groups %llu  stitched %llu  failed %llu\n", what, ok ? "ok  " : "FAIL", gz.size(),
           text.size(), section, (unsigned long long)dev_acc, (unsigned long long)host_acc, (unsigned long long)bridged, (unsigned long long)off.candidates, (unsigned long long)off.groups, (unsigned long long)off.stitched_blocks,
           (unsigned long long)off.failed_blocks);
    if (!ok) ++failures;
    return ok;
}

}  // namespace

// gzb_selftest FILE.gz TEXT [section [group [ratio_cap [tok_ratio]]]]: one single-member file through the emulation with the kernels' own slice budget
static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    {
        // the computed length / distance bases against RFC 1951's tables
        static const uint16_t LB[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const uint8_t LX[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        static const uint16_t DB[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        static const uint8_t DX[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        for (uint32_t i = 0; i < 29; ++i)
            if (len_base(i) != LB[i] || len_extra(i) != LX[i]) { printf("length symbol %u: base / extra wrong\n", i); return 1; }
        for (uint32_t i = 0; i < 30; ++i)
            if (dist_base(i) != DB[i] || dist_extra(i) != DX[i]) { printf("distance symbol %u: base / extra wrong\n", i); return 1; }
    }
    if (argc > 2) {
        const std::vector<uint8_t> gz = slurp(argv[1]), text = slurp(argv[2]);
        g_max_slices = 6; g_slice_tokens = 2048;          // (DeviceInflate::run_group's defaults: slices, 1 token entry per compressed byte, resident results)
        g_tok_ratio = argc > 6 ? (uint32_t)atoi(argv[6]) : 1;
        g_resident = true;
        const bool ok = run_case(argv[1], gz, text, argc > 3 ? (size_t)atol(argv[3]) : 65536, argc > 4 ? (size_t)atol(argv[4]) : 1 << 20, 4, true, argc > 5 ? (uint32_t)atoi(argv[5]) : 12);
        return ok ? 0 : 1;
    }
    // `gzb_selftest 0` / `gzb_selftest 1`: one of the two modes only (the test runs them as two processes side by side)
    const int only_mode = argc == 2 ? atoi(argv[1]) : -1;
    for (int mode = 0; mode < 2; ++mode) {
    if (only_mode >= 0 && mode != only_mode) continue;
    // every case twice: the symbols come back to the host (mode 0, rounds 4 - 5), or stay with the decoder, which resolves their
    // markers and CRCs when the consumer arrives (mode 1, round 6: what DeviceInflate does)
    g_resident = mode == 1;
    printf("---- %s ----\n", g_resident ? "resident results: markers and CRC-32 resolved by the decoder" : "symbols handed back to the host");
    const std::vector<uint8_t> fq = fastq_like(14000, 3);        // ~4.9 MB
    // dynamic-Huffman streams of every level: the device must supply sections
    for (int level : {1, 2, 4, 6, 9}) {
        const std::vector<uint8_t> gz = gz_of(fq, level, Z_DEFAULT_STRATEGY);
        char what[80];
        snprintf(what, sizeof(what), "fastq level %d, 64 KiB sections", level);
        run_case(what, gz, fq, 64 << 10, 512 << 10, 3, true);
    }
    {
        const std::vector<uint8_t> gz = gz_of(fq, 6, Z_DEFAULT_STRATEGY);
        run_case("fastq level 6, 256 KiB sections, one group", gz, fq, 256 << 10, 64 << 20, 2, true);
        run_case("fastq level 6, no host threads", gz, fq, 128 << 10, 1 << 20, 0, true);
        run_case("fastq level 6, symbol space 2x (overflow)", gz, fq, 64 << 10, 512 << 10, 2, false, 2);
        run_case("fastq level 6, 8 candidates per MiB", gz, fq, 64 << 10, 512 << 10, 2, false, 20, 1u << 30);
        g_max_slices = 3;
        run_case("fastq level 6, decoder cut off after 3 slices", gz, fq, 64 << 10, 512 << 10, 2, false);
        g_max_slices = 1u << 20;
        std::vector<uint8_t> bad = gz;
        bad[bad.size() / 2] ^= 0x21;
        run_case("fastq level 6, one byte damaged", bad, fq, 64 << 10, 512 << 10, 2, false, 20, 4096, true);
        std::vector<uint8_t> cut(gz.begin(), gz.begin() + (long)(gz.size() * 2 / 3));
        run_case("fastq level 6, truncated", cut, fq, 64 << 10, 512 << 10, 2, false, 20, 4096, true);
    }
    run_case("fastq huffman-only", gz_of(fq, 6, Z_HUFFMAN_ONLY), fq, 64 << 10, 512 << 10, 2, true);
    run_case("fastq run-length", gz_of(fq, 6, Z_RLE), fq, 64 << 10, 512 << 10, 2, true);
    run_case("fastq fixed codes (host only)", gz_of(fq, 6, Z_FIXED), fq, 64 << 10, 512 << 10, 2, false);
    run_case("fastq stored (host only)", gz_of(fq, 0, Z_DEFAULT_STRATEGY), fq, 64 << 10, 512 << 10, 2, false);
    // pigz-style: an empty stored block between the deflate blocks every 128 KiB of text; and sync flushes
    run_case("fastq level 6, full flush every 128 KiB", gz_of(fq, 6, Z_DEFAULT_STRATEGY, 128 << 10, Z_FULL_FLUSH), fq, 64 << 10, 512 << 10, 2, true);
    run_case("fastq level 1, sync flush every 40 KB", gz_of(fq, 1, Z_DEFAULT_STRATEGY, 40000, Z_SYNC_FLUSH), fq, 64 << 10, 512 << 10, 2, true);
    {
        // concatenated members of different levels + zero padding behind the last one
        std::vector<uint8_t> cat, text;
        int lv = 1;
        for (size_t a = 0; a < fq.size(); a += fq.size() / 3 + 1) {
            std::vector<uint8_t> part(fq.begin() + (long)a, fq.begin() + (long)std::min(fq.size(), a + fq.size() / 3 + 1));
            const std::vector<uint8_t> g = gz_of(part, lv, Z_DEFAULT_STRATEGY);
            cat.insert(cat.end(), g.begin(), g.end());
            text.insert(text.end(), part.begin(), part.end());
            lv += 4;
        }
        cat.insert(cat.end(), 100, 0);
        run_case("three members (levels 1, 5, 9) + zero padding", cat, text, 64 << 10, 512 << 10, 2, true);
    }
    {
        // data in which block headers are easy to mistake: random bytes (stored by zlib), long runs, a tiny alphabet
        std::mt19937 rng(9);
        std::vector<uint8_t> r(1500000);
        for (auto& b : r) b = (uint8_t)rng();
        run_case("random bytes level 6", gz_of(r, 6, Z_DEFAULT_STRATEGY), r, 64 << 10, 512 << 10, 2, false);
        std::vector<uint8_t> runs;
        while (runs.size() < 3000000) { const int k = 1 + (int)(rng() % 900); runs.insert(runs.end(), (size_t)k, (uint8_t)('a' + rng() % 3)); }
        run_case("long runs level 6 (ratio > 20: overflow)", gz_of(runs, 6, Z_DEFAULT_STRATEGY), runs, 64 << 10, 512 << 10, 2, false);
        run_case("long runs level 6, symbol space 400x", gz_of(runs, 6, Z_DEFAULT_STRATEGY), runs, 64 << 10, 512 << 10, 2, false, 400);
        std::vector<uint8_t> two(2000000);
        for (auto& b : two) b = (uint8_t)("AC"[rng() & 1]);
        run_case("two-symbol text level 9", gz_of(two, 9, Z_DEFAULT_STRATEGY), two, 64 << 10, 512 << 10, 2, true);
        std::vector<uint8_t> one(1, 'x'), none;
        run_case("one byte", gz_of(one, 6, Z_DEFAULT_STRATEGY), one, 64 << 10, 512 << 10, 2, false);
        run_case("empty", gz_of(none, 6, Z_DEFAULT_STRATEGY), none, 64 << 10, 512 << 10, 2, false);
    }
    {
        const std::vector<uint8_t> big = fastq_like(60000, 11);   // ~21 MB: several groups of 2 MiB, distances near 32 KiB do occur at level 9
        run_case("fastq 21 MB level 9, 256 KiB sections", gz_of(big, 9, Z_DEFAULT_STRATEGY), big, 256 << 10, 2 << 20, 4, true);
        run_case("fastq 21 MB level 1, 1 MiB sections", gz_of(big, 1, Z_DEFAULT_STRATEGY), big, 1 << 20, 4 << 20, 4, true);
    }
    {
        // HYBRID: the pool takes the window's sections from the bottom up, the device groups from the top down (what the pipe runs)
        const std::vector<uint8_t> big = fastq_like(60000, 12);
        const std::vector<uint8_t> g6 = gz_of(big, 6, Z_DEFAULT_STRATEGY), g1 = gz_of(big, 1, Z_DEFAULT_STRATEGY);
        run_case("hybrid: 21 MB level 6, 64 KiB sections, groups of 4", g6, big, 64 << 10, 256 << 10, 3, true, 20, 4096, false, true);
        run_case("hybrid: 21 MB level 1, 128 KiB sections, groups of 8", g1, big, 128 << 10, 1 << 20, 2, true, 20, 4096, false, true);
        run_case("hybrid: 21 MB level 6, no pool threads", g6, big, 64 << 10, 512 << 10, 0, true, 20, 4096, false, true);
        run_case("hybrid: full flush every 128 KiB", gz_of(big, 6, Z_DEFAULT_STRATEGY, 128 << 10, Z_FULL_FLUSH), big, 64 << 10, 256 << 10, 3, true, 20, 4096, false, true);
        std::vector<uint8_t> bad = g6;
        bad[bad.size() / 3] ^= 0x44;
        run_case("hybrid: one byte damaged", bad, big, 64 << 10, 256 << 10, 3, false, 20, 4096, true, true);
        const std::vector<uint8_t> small = fastq_like(300, 13);
        run_case("hybrid: 100 KB file", gz_of(small, 6, Z_DEFAULT_STRATEGY), small, 64 << 10, 256 << 10, 2, false, 20, 4096, false, true);
        // the device gives up (its first / its third group fails, it takes no more work): the host decodes on, in both modes — the
        // device-only mode used to wait forever for a section nobody would make (round-4 advisory)
        g_break_after = 0;
        run_case("device breaks at group 1 (device only)", g6, big, 64 << 10, 256 << 10, 3, false);
        run_case("device breaks at group 1 (device only, no pool)", g6, big, 64 << 10, 256 << 10, 0, false);
        run_case("device breaks at group 1 (hybrid)", g6, big, 64 << 10, 256 << 10, 3, false, 20, 4096, false, true);
        g_break_after = 2;
        run_case("device breaks at group 3 (device only)", g6, big, 64 << 10, 256 << 10, 3, true);
        run_case("device breaks at group 3 (hybrid)", g1, big, 128 << 10, 1 << 20, 2, false, 20, 4096, false, true);
        g_break_after = -1;
        if (g_resident) {
            // the decoder fails when asked to resolve (a HIP error at that point): the run's sections are dropped, the host decodes the stretch
            g_resolve_breaks_after = 1;
            run_case("resolve fails from the 2nd run on (device only)", g6, big, 64 << 10, 256 << 10, 3, true);
            run_case("resolve fails from the 2nd run on (hybrid)", g6, big, 64 << 10, 256 << 10, 3, true, 20, 4096, false, true);
            g_resolve_breaks_after = -1;
            // a member that starts less than 32 KiB before a device section: window entries that do not exist
            std::vector<uint8_t> cat, text;
            const std::vector<uint8_t> head = fastq_like(40, 21);
            const std::vector<uint8_t> g0 = gz_of(head, 6, Z_DEFAULT_STRATEGY);
            cat.insert(cat.end(), g0.begin(), g0.end()); text.insert(text.end(), head.begin(), head.end());
            cat.insert(cat.end(), g6.begin(), g6.end()); text.insert(text.end(), big.begin(), big.end());
            run_case("short member, then a long one", cat, text, 64 << 10, 256 << 10, 3, true);
        }
    }
    }
    // (only the resident mode resolves sections and hands over segments)
    if (only_mode != 0 && g_sections_resolved == 0) { printf("no section was ever resolved by the emulated device\n"); ++failures; }
    if (only_mode != 0 && g_segment_bytes == 0) { printf("no text was ever handed over as a device segment\n"); ++failures; }
    printf("%.1f MB of text handed over as device segments\n", 1e-6 * (double)g_segment_bytes);
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("all device-gunzip logic checks passed\n");
    return 0;
}
