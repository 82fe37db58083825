// bzb_selftest — csrc/aqc_bunzip2_dev.hpp on the CPU: the functions a lane of the device bunzip2 runs (block scan, entropy
// stage, inverse BWT, RLE1 + CRC, chain), compiled with the host compiler and dealt out by plain loops through the same
// aqcbz::decode_stream (csrc/aqc_bz2.hpp) that drives the device.  No GPU, no HIP.
//
//   bzb_selftest <manifest>
// a line of the manifest:  <file.bz2> <file with the expected text, or - > <window bytes> <group blocks> <text bytes per group> <exact|handback|error>
//   exact: the file decodes to the expected text and NO block was handed back to libbz2;  handback: the expected text, and at
//   least one block was handed back (libbz2 finished the stream);  error: a negative status.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../afterqc_amd/csrc/aqc_bunzip2_dev.hpp"
#include "../../afterqc_amd/csrc/aqc_bz2.hpp"

using namespace aqc;

namespace {

std::vector<uint8_t> slurp(const char* path, bool* ok) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    *ok = f != nullptr;
    if (!f) return v;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

// the device's candidate list holds as many (aqc_bunzip2_offload.hip: BZB_CAND_CAP)
constexpr size_t CAND_CAP = 65536;

// what DeviceBunzip2 does with kernels, with loops
struct CpuBlocks {
    size_t group_size = 4;
    uint64_t out_cap = 640u << 20;
    std::vector<uint8_t> comp, text, sel;
    std::vector<uint64_t> cand;
    uint64_t nbits = 0;
    uint32_t crc_tab[256];
    CpuBlocks() { for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = bzb_crc_entry(i); }
    size_t default_group(uint32_t) const { return group_size; }
    bool scan(const uint8_t* win, size_t wlen, std::vector<uint64_t>& cands, bool* overflow) {
        comp.assign(win, win + wlen);
        comp.resize(wlen + BZB_PAD, 0);
        nbits = (uint64_t)wlen * 8u;
        cands.clear();
        for (uint64_t word = 0; word * 64u < nbits; ++word) {
            uint64_t mb, me;
            bzb_scan64(comp.data(), nbits, word * 8u, &mb, &me);
            for (uint32_t s = 0; s < 64u; ++s)
                if (((mb | me) >> s) & 1ull) cands.push_back(((word * 64u + s) << 1) | ((me >> s) & 1ull));
        }
        // (more hits than the device's list holds: incomplete there, so not used here either — as DeviceBunzip2::try_scan)
        *overflow = cands.size() > CAND_CAP;
        if (*overflow) cands.clear();
        cand = cands;
        return true;
    }
    bool group(size_t first, size_t g, uint64_t cur, uint32_t level, aqcbz::GroupResult& R) {
        const uint32_t slot = (level * 100000u + 15u) & ~15u;
        // (fresh and exactly sized for every group, so that the sanitizer build sees a step outside a slot; not zeroed — a
        //  stream of tens of thousands of tiny blocks would spend its time there: every byte is written before it is read)
        const std::unique_ptr<uint8_t[]> bw(new uint8_t[g * (size_t)slot]);
        const std::unique_ptr<uint32_t[]> tt(new uint32_t[slot]);
        std::vector<uint32_t> counts(g * 256u), idx(g), cf(256);
        std::vector<uint64_t> off(g + 1);
        std::vector<BzbBlock> blk(g);
        sel.resize(BZB_SEL_BYTES);
        for (size_t c = 0; c < g; ++c) {
            BzbBlock& b = blk[c];
            if (cand[first + c] & 1ull) { b = BzbBlock{}; b.status = BZB_EOS; continue; }
            BzbTables T;
            bzb_entropy_block(comp.data(), nbits, cand[first + c] >> 1, level, T, sel.data(), bw.get() + c * slot, counts.data() + c * 256u, &b);
            if (b.status != BZB_OK) continue;
            if (!bzb_bwt_scatter(bw.get() + c * slot, tt.get(), b.nblock, b.orig_ptr, counts.data() + c * 256u, cf.data()) ||
                !bzb_bwt_chase(bw.get() + c * slot, tt.get(), b.nblock, b.orig_ptr)) { b.status = BZB_BAD; continue; }
            b.out_size = bzb_rle1_size(bw.get() + c * slot, b.nblock);
            if (b.out_size == BZB_NO_SIZE) { b.out_size = 0; b.status = BZB_BAD; }
        }
        BzbChain ch;
        bzb_chain(cand.data() + first, (uint32_t)g, blk.data(), cur, out_cap, &ch, idx.data(), off.data());
        R.n = ch.n; R.stop_status = ch.stop_status;
        R.crc_hdr.resize(ch.n); R.crc_txt.resize(ch.n); R.end_bit.resize(ch.n); R.off.assign(off.begin(), off.begin() + ch.n + 1);
        text.assign((size_t)ch.total + 64, 0xEE);
        for (uint32_t k = 0; k < ch.n; ++k) {
            const BzbBlock& b = blk[idx[k]];
            uint64_t written = 0;
            const uint32_t crc = bzb_rle1_write(bw.get() + (size_t)idx[k] * slot, b.nblock, text.data() + off[k], off[k + 1] - off[k], crc_tab, &written);
            R.crc_hdr[k] = b.crc; R.end_bit[k] = b.end_bit;
            R.crc_txt[k] = written == off[k + 1] - off[k] ? crc : ~b.crc;
        }
        R.text = text.data();
        return true;
    }
};

// one file image, as aqc_bunzip2_dev walks it
int decode_file(const std::vector<uint8_t>& bz, size_t window, size_t group, uint64_t out_cap, std::vector<uint8_t>& text, aqcbz::StreamStats& st) {
    if (bz.empty()) return 0;
    std::vector<size_t> starts;
    aqcbz::stream_starts(bz.data(), bz.size(), starts);
    if (starts.size() < 2 || starts[0] != 0) return -9;
    CpuBlocks B;
    B.group_size = group ? group : 4;
    B.out_cap = out_cap;
    const aqcbz::Sink sink = [&](const uint8_t* p, size_t n) { text.insert(text.end(), p, p + n); return true; };
    for (size_t k = 0; k + 1 < starts.size(); ++k) {
        size_t end = starts[k + 1];
        const int rc = aqcbz::decode_stream(B, bz.data(), starts[k], starts[k + 1], window, B.group_size, sink, &end, st, nullptr);
        if (rc != 0) return rc;
        if (end != starts[k + 1]) break;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: bzb_selftest <manifest>\n"); return 2; }
    FILE* mf = fopen(argv[1], "r");
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    if (!aqcbz::Bz2Api::get().ok) { fprintf(stderr, "libbz2 could not be loaded\n"); return 2; }
    char a[1024], b[1024], want[32];
    unsigned long long window, group, out_cap;
    int failures = 0, cases = 0;
    while (fscanf(mf, "%1023s %1023s %llu %llu %llu %31s", a, b, &window, &group, &out_cap, want) == 6) {
        bool ok1 = true, ok2 = true;
        const std::vector<uint8_t> bz = slurp(a, &ok1);
        const std::vector<uint8_t> plain = strcmp(b, "-") ? slurp(b, &ok2) : std::vector<uint8_t>();
        if (!ok1 || !ok2) { printf("FAIL %s: cannot read the inputs\n", a); ++failures; continue; }
        std::vector<uint8_t> text;
        aqcbz::StreamStats st;
        const int rc = decode_file(bz, (size_t)window, (size_t)group, out_cap, text, st);
        bool good;
        if (!strcmp(want, "error")) good = rc < 0;
        else if (!strcmp(want, "handback")) good = rc == 0 && text == plain && st.host_blocks >= 1;
        else if (!strcmp(want, "exact")) good = rc == 0 && text == plain && st.host_blocks == 0 && st.dev_bytes == text.size();
        else good = false;
        printf("%s %s: window %llu group %llu — rc %d, %zu bytes of text (expected %zu), %llu blocks decoded by the emulated device, %llu handed back\n", good ? "ok  " : "FAIL", a,
               window, group, rc, text.size(), plain.size(), (unsigned long long)st.dev_blocks, (unsigned long long)st.host_blocks);
        failures += good ? 0 : 1;
        ++cases;
    }
    fclose(mf);
    if (failures || !cases) { printf("%d of %d cases FAILED\n", failures, cases); return 1; }
    printf("all %d device-bunzip2 logic checks passed\n", cases);
    return 0;
}
