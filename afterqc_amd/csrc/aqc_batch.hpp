// aqc_batch.hpp — a batch as it sits in HBM and what every stage shares about it: the batch / circle / statistics / k-mer table
// descriptors, how a device error is raised at a record, and the workgroup-private counters and their flush.  It defines no kernel:
// every C-API unit includes it (through aqc_ctx.hpp: the context and its slots are made of these descriptors).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"

namespace aqc {

struct DevBatch {
    const uint8_t *seq1, *qual1, *seq2, *qual2;
    const uint32_t *off1, *qoff1, *off2, *qoff2;   // byte offsets into the arenas (a chunk / batch arena is < 4 GiB); qoff NULL = off
    const uint32_t *len1, *len2;
    const int32_t *aux_lane, *aux_tile, *aux_x, *aux_y;
    const uint8_t* aux_ok;
    uint64_t n;
    uint64_t first_index;
    // Records whose QUALITY line is not as long as their SEQUENCE line (the reference never compares the two: fastq.py:37-49
    // hands the lines over as they are, preprocesser.py:19-28 slices each string by its own length, :565-568 index each quality
    // string from its own end).  Such a mate carries LEN_IRR in its len word; qlen holds the quality line's length (low 31
    // bits; NULL: the batch has no such record) and the general kernel leaves the FINAL quality view of both mates of such a
    // record in qview (start | length << 16, relative to the quality line) for the writer and the post-filter statRead.
    const uint32_t *qlen1, *qlen2;
    uint32_t *qview1, *qview2;
};
constexpr uint32_t LEN_IRR = 0x80000000u, LEN_MASK = 0x7fffffffu;
// the quality-length words of a framed chunk (frame_records_kernel) carry two flags above the length: the quality line ends right
// at its '\n' (nothing stripped), and ALL FOUR lines of the record do — the record stands in the chunk exactly as a writer would
// write it
constexpr uint32_t QLEN_TAILNL = 0x80000000u, QLEN_CONTIG = 0x40000000u, QLEN_MASK = 0x3fffffffu;

struct DevCircles {
    const double *cx, *cy, *cr;
    const int32_t *lane, *tile;
    int32_t n;
};

struct DevStats {
    unsigned long long* counters;   // [AQC_N_COUNTERS]
    unsigned long long* ovl_hist;   // [AQC_QC_COLS]
    unsigned long long* dist_hist;  // [AQC_QC_COLS]
    int* status;                    // first error code raised on the device (0 = ok)
    // errors that END THE RUN AT A RECORD upstream (an exception inside the loop of preprocesser.py:411-631: KeyError of
    // util.complement / the error matrix, IndexError of a quality string too short for the walk, int() of a name field):
    // min over (record << 8 | -code), so that the host learns the EARLIEST such record — everything before it was written
    // upstream when the exception flew (~0 = none)
    unsigned long long* err_key;
};
__device__ __forceinline__ void raise_at_record(const DevStats& st, uint64_t rec, int code) {
    atomicCAS(st.status, 0, code);
    atomicMin(st.err_key, ((unsigned long long)rec << 8) | (unsigned long long)(unsigned int)(-code));
}

struct BlockAcc {
    unsigned long long counters[AQC_N_COUNTERS];
    unsigned int ovl_hist[AQC_QC_COLS];
    unsigned int dist_hist[AQC_QC_COLS];
};

// block-private counters -> the device's, once per workgroup
__device__ inline void flush_block_acc(BlockAcc& acc, const DevStats& st, int tid = -1) {
    if (tid < 0) tid = (int)threadIdx.x;
    for (int i = tid; i < AQC_N_COUNTERS; i += blockDim.x)
        if (acc.counters[i]) atomicAdd(&st.counters[i], acc.counters[i]);
    for (int i = tid; i < AQC_QC_COLS; i += blockDim.x) {
        if (acc.ovl_hist[i]) atomicAdd(&st.ovl_hist[i], (unsigned long long)acc.ovl_hist[i]);
        if (acc.dist_hist[i]) atomicAdd(&st.dist_hist[i], (unsigned long long)acc.dist_hist[i]);
    }
}

// the k-mer dictionary of one statRead accumulator (the kernels: aqc_qcstat.hpp), a member of the context
struct KmerTable {
    // open-addressing table for k-mers containing anything but A,C,G,T (rare): keyed by the k raw bytes
    unsigned long long* keys;    // 0 = empty
    unsigned long long* counts;  // [capacity + 1]: entry `capacity` belongs to the all-NUL k-mer, whose key is 0 (see kmer_slot)
    unsigned long long* order;   // [capacity + 1] min over 2*t (seen) / 2*t+1 (inserted as reverse complement)
    uint64_t mask;               // capacity - 1
    // dense tables for pure A/C/G/T k-mers, 4^k entries.  Index = (bit-1 plane << k) | bit-0 plane of the
    // per-base code (c >> 1) & 3 (A=0 C=1 T=2 G=3); base j of the k-mer sits at bit j of each plane.
    // One copy of the dense tables PER XCD (8 on MI355X): a wave updates the copy of the XCD it runs on with
    // atomics that execute in that XCD's L2 (workgroup scope is enough: every accessor of a copy shares the L2),
    // instead of device-scope atomics that have to travel to the memory side.  Copies are summed / min-ed when
    // the dictionary is read back.
    unsigned int* dense_count;         // [N_XCD][4^k]
    unsigned long long* dense_first;   // [N_XCD][4^k] smallest scan time t at which the k-mer was seen (~0 = never)
    // complete[b] != 0: every dense entry of reduce-workgroup b has a first-seen time (written by kmer_reduce_kernel).
    // Time keys only grow from launch to launch, so once every entry has one no later launch can lower any of them
    // and kmer_count_kernel stops probing the first-seen table (for random DNA that is after ~10^4 reads).
    unsigned int* complete;            // [DENSE_ENTRIES / KRED_ENTRIES]
};
constexpr int N_XCD = 8;
constexpr uint32_t DENSE_ENTRIES = 1u << 16;   // 4^8
constexpr int KRED_ENTRIES = 256;       // dense entries per kmer_reduce_kernel workgroup

}  // namespace aqc
