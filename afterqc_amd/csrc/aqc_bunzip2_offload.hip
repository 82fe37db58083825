// aqc_bunzip2_offload.hip — bzip2 INPUT on the device: the host driver of the kernels in aqc_bunzip2_dev.hpp.
//
// DeviceBunzip2 is the block decoder that aqcbz::decode_stream (aqc_bz2.hpp) drives — a window of the compressed stream is
// uploaded and scanned, its candidates go through entropy -> BWT -> chain -> expand in groups, a group's text comes back
// contiguous and in stream order — and the aqcbz::StreamDecoder the pipe's Bz2Source hands its big streams to;
// aqc_bunzip2_dev is the C entry that decodes one whole file image with it.  A unit of its own, like aqc_gunzip_offload.hip:
// of the C ABI it needs only the page-locked host memory.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "aqc_dev.hpp"
#include "aqc_bunzip2_dev.hpp"
#include "aqc_bz2.hpp"
#include "aqc_keep.hpp"

using namespace aqc;

namespace {

std::atomic<uint64_t> g_bzb_stats[7];      // microseconds: scan + sort, entropy, BWT (scatter + chase + sizes + chain), expand, copies; of the BWT figure: scatter, chase (process-wide)

// Device memory of one decoder.  A block in flight takes 5 bytes per byte of its level x 100,000 (the BWT bytes, later the
// chased bytes, and the successor vector's words) + 18 KB of selectors; a gunzip decoder may take 2.5 GB,
// and so may this one: a window of <= 128 MiB compressed, text of <= 640 MiB per group, 1.7 GB of blocks — 375 at level 9.
constexpr size_t BZB_WINDOW = 128u << 20, BZB_OUT_CAP = 640u << 20, BZB_BLOCK_BUDGET = 1700u << 20;
constexpr uint32_t BZB_CAND_CAP = 65536u;

class DeviceBunzip2 : public aqcbz::StreamDecoder {
public:
    DeviceBunzip2(int device, size_t group_blocks) : device_(device), group_blocks_(group_blocks) {}
    // (runs when a pipe drops a decoder that gave up or that the keeper had no room for — never at exit(): aqc_keep.hpp)
    ~DeviceBunzip2() override {
        (void)hipSetDevice(device_);
        if (stream_) (void)hipStreamSynchronize(stream_);
        for (DevBuf* x : all()) x->release();
        for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
        if (stream_) (void)hipStreamDestroy(stream_);
        if (pin_) aqc_host_free(pin_);
        if (meta_) aqc_host_free(meta_);
    }
    bool start() {
        if (hipSetDevice(device_) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) return false;
        for (auto& e : ev_) if (hipEventCreate(&e) != hipSuccess) return false;
        return true;
    }
    bool gave_up() override { return broken_.load(); }
    int decode(const uint8_t* data, size_t a, size_t b, const aqcbz::Sink& sink, size_t* end_byte, aqcbz::StreamStats* st, const std::atomic<bool>* stop) override {
        std::lock_guard<std::mutex> g(mu_);
        aqcbz::StreamStats local;
        aqcbz::StreamStats& S = st ? *st : local;
        if (broken_) {
            uint64_t produced = 0;
            const int rc = aqcbz::host_decode(data, a, b, 0, sink, end_byte, &produced, stop);
            S.host_blocks += 1; S.host_bytes += produced;
            return rc;
        }
        return aqcbz::decode_stream(*this, data, a, b, BZB_WINDOW, group_blocks_, sink, end_byte, S, stop);
    }

    // ---- what aqcbz::decode_stream drives ----------------------------------------------------------------------------------------
    size_t default_group(uint32_t level) const { return std::max<size_t>(1, BZB_BLOCK_BUDGET / (5ull * slot_of(level) + BZB_SEL_BYTES + 1024u + sizeof(BzbBlock))); }
    bool scan(const uint8_t* win, size_t wlen, std::vector<uint64_t>& cands, bool* overflow) {
        cands.clear();
        if (!try_scan(win, wlen, cands, overflow)) { (void)hipGetLastError(); broken_ = true; return false; }
        return true;
    }
    bool group(size_t first, size_t g, uint64_t cur, uint32_t level, aqcbz::GroupResult& R) {
        if (!try_group(first, g, cur, level, R)) { (void)hipGetLastError(); broken_ = true; return false; }
        return true;
    }

private:
#define BZB_TRY(expr) do { if ((expr) != hipSuccess) return false; } while (0)
    static uint32_t slot_of(uint32_t level) { return (level * 100000u + 15u) & ~15u; }
    std::vector<DevBuf*> all() { return {&comp_, &cand_raw_, &cand_, &n_cand_, &sel_, &bw_, &tt_, &counts_, &blk_, &chain_, &out_}; }
    void add_us(int i, hipEvent_t a, hipEvent_t b) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess) g_bzb_stats[i] += (uint64_t)(ms * 1000.0f);
    }
    bool reserve_pin(uint8_t*& p, size_t& cap, size_t need) {
        if (cap >= need) return true;
        if (p) aqc_host_free(p);
        cap = need + need / 4 + (1u << 20);
        p = (uint8_t*)aqc_host_alloc(cap);
        if (!p) { cap = 0; return false; }
        return true;
    }
    bool try_scan(const uint8_t* win, size_t wlen, std::vector<uint64_t>& cands, bool* overflow) {
        BZB_TRY(hipSetDevice(device_));
        if (comp_.reserve(wlen + BZB_PAD) || cand_raw_.reserve(8ull * BZB_CAND_CAP) || cand_.reserve(8ull * BZB_CAND_CAP) || n_cand_.reserve(64)) return false;
        if (!reserve_pin(meta_, meta_cap_, 8ull * BZB_CAND_CAP + 64)) return false;
        BZB_TRY(hipEventRecord(ev_[0], stream_));
        BZB_TRY(hipMemcpyAsync(comp_.p, win, wlen, hipMemcpyHostToDevice, stream_));
        BZB_TRY(hipMemsetAsync((uint8_t*)comp_.p + wlen, 0, BZB_PAD, stream_));
        BZB_TRY(hipMemsetAsync(n_cand_.p, 0, 64, stream_));
        BZB_TRY(hipEventRecord(ev_[1], stream_));
        J_ = BzbJob{};
        J_.comp = (const uint8_t*)comp_.p; J_.nbits = (uint64_t)wlen * 8u;
        J_.cand_raw = (uint64_t*)cand_raw_.p; J_.cand = (uint64_t*)cand_.p; J_.n_cand = (uint32_t*)n_cand_.p; J_.cand_cap = BZB_CAND_CAP;
        const uint64_t words = ((uint64_t)wlen + 7u) / 8u;
        hipLaunchKernelGGL(bzb_scan_kernel, dim3((unsigned)((words + BZB_SCAN_THREADS - 1) / BZB_SCAN_THREADS)), dim3(BZB_SCAN_THREADS), 0, stream_, J_);
        BZB_TRY(hipGetLastError());
        BZB_TRY(hipMemcpyAsync(meta_, n_cand_.p, 4, hipMemcpyDeviceToHost, stream_));
        BZB_TRY(hipStreamSynchronize(stream_));
        const uint32_t n = *(const uint32_t*)meta_;
        *overflow = n > BZB_CAND_CAP;
        if (n && !*overflow) {
            hipLaunchKernelGGL(bzb_sort_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream_, J_);
            BZB_TRY(hipGetLastError());
        }
        BZB_TRY(hipEventRecord(ev_[2], stream_));
        if (n && !*overflow) BZB_TRY(hipMemcpyAsync(meta_, cand_.p, 8ull * n, hipMemcpyDeviceToHost, stream_));
        BZB_TRY(hipEventRecord(ev_[3], stream_));
        BZB_TRY(hipStreamSynchronize(stream_));
        if (n && !*overflow) cands.assign((const uint64_t*)meta_, (const uint64_t*)meta_ + n);
        add_us(4, ev_[0], ev_[1]); add_us(0, ev_[1], ev_[2]); add_us(4, ev_[2], ev_[3]);
        return true;
    }
    bool try_group(size_t first, size_t g, uint64_t cur, uint32_t level, aqcbz::GroupResult& R) {
        BZB_TRY(hipSetDevice(device_));
        const uint32_t slot = slot_of(level);
        const size_t o_idx = sizeof(BzbChain), o_off = (o_idx + 4 * g + 7) & ~(size_t)7, o_crc = o_off + 8 * (g + 1), chain_bytes = (o_crc + 4 * g + 7) & ~(size_t)7;
        if (sel_.reserve(g * (size_t)BZB_SEL_BYTES) || bw_.reserve(g * (size_t)slot) || tt_.reserve(4ull * g * slot) || counts_.reserve(1024ull * g) ||
            blk_.reserve(sizeof(BzbBlock) * g) || chain_.reserve(chain_bytes))
            return false;
        if (!reserve_pin(meta_, meta_cap_, std::max<size_t>(8ull * BZB_CAND_CAP + 64, chain_bytes + sizeof(BzbBlock) * g))) return false;
        BzbJob& J = J_;
        J.first = (uint32_t)first; J.g = (uint32_t)g; J.level = level; J.slot = slot;
        J.sel = (uint8_t*)sel_.p; J.bw = (uint8_t*)bw_.p; J.tt = (uint32_t*)tt_.p; J.counts = (uint32_t*)counts_.p; J.blk = (BzbBlock*)blk_.p;
        J.cur = cur; J.out_cap = BZB_OUT_CAP;
        J.chain = (BzbChain*)chain_.p; J.chain_idx = (uint32_t*)((uint8_t*)chain_.p + o_idx); J.chain_off = (uint64_t*)((uint8_t*)chain_.p + o_off);
        J.crc_out = (uint32_t*)((uint8_t*)chain_.p + o_crc);
        BZB_TRY(hipEventRecord(ev_[0], stream_));
        hipLaunchKernelGGL(bzb_entropy_kernel, dim3((unsigned)g), dim3(64), 0, stream_, J);
        BZB_TRY(hipEventRecord(ev_[1], stream_));
        hipLaunchKernelGGL(bzb_scatter_kernel, dim3((unsigned)g), dim3(64), 0, stream_, J);
        BZB_TRY(hipEventRecord(ev_[4], stream_));
        hipLaunchKernelGGL(bzb_chase_kernel, dim3((unsigned)g), dim3(64), 0, stream_, J);
        BZB_TRY(hipEventRecord(ev_[5], stream_));
        hipLaunchKernelGGL(bzb_size_kernel, dim3((unsigned)g), dim3(64), 0, stream_, J);
        hipLaunchKernelGGL(bzb_chain_kernel, dim3(1), dim3(64), 0, stream_, J);
        BZB_TRY(hipGetLastError());
        BZB_TRY(hipEventRecord(ev_[2], stream_));
        BZB_TRY(hipMemcpyAsync(meta_, chain_.p, o_crc, hipMemcpyDeviceToHost, stream_));
        BZB_TRY(hipMemcpyAsync(meta_ + chain_bytes, blk_.p, sizeof(BzbBlock) * g, hipMemcpyDeviceToHost, stream_));
        BZB_TRY(hipEventRecord(ev_[3], stream_));
        BZB_TRY(hipStreamSynchronize(stream_));
        const BzbChain ch = *(const BzbChain*)meta_;
        const uint32_t* idx = (const uint32_t*)(meta_ + o_idx);
        const uint64_t* off = (const uint64_t*)(meta_ + o_off);
        const BzbBlock* blk = (const BzbBlock*)(meta_ + chain_bytes);
        if (ch.n > g) return false;
        R.n = ch.n; R.stop_status = ch.stop_status; R.text = nullptr;
        R.crc_hdr.resize(ch.n); R.crc_txt.resize(ch.n); R.end_bit.resize(ch.n); R.off.assign(off, off + ch.n + 1);
        for (uint32_t k = 0; k < ch.n; ++k) { R.crc_hdr[k] = blk[idx[k]].crc; R.end_bit[k] = blk[idx[k]].end_bit; }
        add_us(1, ev_[0], ev_[1]); add_us(2, ev_[1], ev_[2]); add_us(4, ev_[2], ev_[3]); add_us(5, ev_[1], ev_[4]); add_us(6, ev_[4], ev_[5]);
        if (!ch.n) return true;
        // the text: a place for it on the device and in page-locked memory, then the runs expanded and the CRCs
        if (out_.reserve((size_t)ch.total + 64) || !reserve_pin(pin_, pin_cap_, (size_t)ch.total + 64)) return false;
        J.out = (uint8_t*)out_.p;
        BZB_TRY(hipEventRecord(ev_[0], stream_));
        hipLaunchKernelGGL(bzb_expand_kernel, dim3(ch.n), dim3(64), 0, stream_, J);
        BZB_TRY(hipGetLastError());
        BZB_TRY(hipEventRecord(ev_[1], stream_));
        BZB_TRY(hipMemcpyAsync(meta_, J.crc_out, 4ull * ch.n, hipMemcpyDeviceToHost, stream_));
        if (ch.total) BZB_TRY(hipMemcpyAsync(pin_, out_.p, (size_t)ch.total, hipMemcpyDeviceToHost, stream_));
        BZB_TRY(hipEventRecord(ev_[2], stream_));
        BZB_TRY(hipStreamSynchronize(stream_));
        memcpy(R.crc_txt.data(), meta_, 4ull * ch.n);
        R.text = pin_;
        add_us(3, ev_[0], ev_[1]); add_us(4, ev_[1], ev_[2]);
        return true;
    }
#undef BZB_TRY

    int device_;
    size_t group_blocks_;
    std::mutex mu_;
    std::atomic<bool> broken_{false};
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[6] = {};
    DevBuf comp_, cand_raw_, cand_, n_cand_, sel_, bw_, tt_, counts_, blk_, chain_, out_;
    BzbJob J_{};
    uint8_t* pin_ = nullptr;
    uint8_t* meta_ = nullptr;
    size_t pin_cap_ = 0, meta_cap_ = 0;
};

// aqc_bunzip2_dev's decoders, lent to its callers for the life of the process (aqc_keep.hpp); keyed by (device, blocks per group)
Keep<std::pair<int, uint64_t>, aqcbz::StreamDecoder>* const g_dev_keep = new Keep<std::pair<int, uint64_t>, aqcbz::StreamDecoder>;

}  // namespace

namespace aqcbz {
StreamDecoder* make_device_bunzip2(int device, size_t group_blocks) {
    std::unique_ptr<DeviceBunzip2> d(new DeviceBunzip2(device, group_blocks));
    if (!d->start()) { (void)hipGetLastError(); return nullptr; }
    return d.release();
}
void device_bunzip2_stats(uint64_t out[7]) {
    for (int i = 0; i < 7; ++i) out[i] = g_bzb_stats[i].load();
}
}  // namespace aqcbz

extern "C" {

// One bzip2 file image decoded with the device taking every block that chains up: every stream of it, as bz2.BZ2File of
// Python 3 does; bytes behind a stream's end that are not a stream end the data there.  stats: blocks decoded on the device /
// handed back to the host, bytes the host decoded, then microseconds in the scan, entropy, BWT and expand kernels and in the
// copies.  A hand-back RESTARTS the stream: libbz2 decodes it from its first byte and the text the device has delivered is
// dropped from its output (aqc_bz2.hpp) — a damaged or randomised block near the end of a big stream costs the whole stream's
// single-thread time on top of the device's.  `threads` is kept for the twin's signature: what the host does here (libbz2 on what is handed back) is one thread.
int aqc_bunzip2_dev(int device, const uint8_t* bz, uint64_t size, uint8_t* out, uint64_t cap, uint64_t* n_out, uint64_t stats[8], int threads,
                    uint64_t group_blocks) {
    (void)threads;
    if ((!bz && size) || (!out && cap) || !n_out || !stats) return fail(AQC_ERR_ARG, "null argument");
    memset(stats, 0, 8 * sizeof(uint64_t));
    *n_out = 0;
    if (!size) return 0;
    if (!aqcbz::Bz2Api::get().ok) return fail(AQC_ERR_ARG, "device bunzip2: libbz2 could not be loaded (the host takes what the device hands back)");
    // (one decoder per device and group size for the life of the process, as aqc_gunzip_dev keeps its own)
    aqcbz::StreamDecoder* dec = g_dev_keep->lend({device, group_blocks}, [&] { return aqcbz::make_device_bunzip2(device, (size_t)group_blocks); });
    if (!dec || dec->gave_up()) return fail(AQC_ERR_HIP, "device bunzip2: cannot set up device %d", device);
    // stream starts, byte aligned, as Bz2Source::produce finds them
    std::vector<size_t> starts;
    aqcbz::stream_starts(bz, (size_t)size, starts);
    if (starts.size() < 2 || starts[0] != 0) return fail(AQC_ERR_ARG, "device bunzip2: not a bzip2 file");
    uint64_t before[7], after[7], produced = 0;
    aqcbz::device_bunzip2_stats(before);
    aqcbz::StreamStats st;
    bool full = false;
    const aqcbz::Sink sink = [&](const uint8_t* p, size_t n) {
        if (n > cap - produced) { full = true; return false; }
        memcpy(out + produced, p, n);
        produced += n;
        return true;
    };
    int rc = 0;
    for (size_t k = 0; k + 1 < starts.size(); ++k) {
        size_t end = starts[k + 1];
        const int r = dec->decode(bz, starts[k], starts[k + 1], sink, &end, &st, nullptr);
        if (r != 0) {
            rc = full ? fail(AQC_ERR_ARG, "output does not fit") : dec->gave_up() ? fail(AQC_ERR_HIP, "device bunzip2: a device call failed")
                                                                                 : fail(AQC_ERR_ARG, "device bunzip2: corrupt or truncated bzip2 stream");
            break;
        }
        if (end != starts[k + 1]) break;       // bytes that are no stream follow: the data ends here
    }
    if (!rc && dec->gave_up()) rc = fail(AQC_ERR_HIP, "device bunzip2: a device call failed");
    aqcbz::device_bunzip2_stats(after);
    stats[0] = st.dev_blocks; stats[1] = st.host_blocks; stats[2] = st.host_bytes;
    for (int i = 0; i < 5; ++i) stats[3 + i] = after[i] - before[i];
    // AQC_BZ2_DEBUG=1: what the BWT figure is made of — the successor chase on its own — on stderr
    if (const char* e = getenv("AQC_BZ2_DEBUG"))
        if (e[0] == '1')
            fprintf(stderr, "[bz2 dev %d] BWT stage %.1f ms = scatter %.1f + chase %.1f + sizes and chain %.1f\n", device, (after[2] - before[2]) / 1e3, (after[5] - before[5]) / 1e3,
                    (after[6] - before[6]) / 1e3, ((after[2] - before[2]) - (after[5] - before[5]) - (after[6] - before[6])) / 1e3);
    *n_out = produced;
    return rc;
}

}  // extern "C"
