"""-m gpu: the statRead kernels (qc_stat_kernel, kmer_count_kernel with its fused per-cycle rows, kmer_reduce_kernel, the two
compaction kernels) against the oracle — every QC row and the whole k-mer dictionary (keys, counts, insertion rank, top k-mers) —
where the small parity batches never go:
  - the full sample: a million pairs in one qc_stat call per object (the multi-launch loop of aqc_qc_stat) and in the CLI's pattern
    of chunked batches;
  - saturated u16 round slices (homopolymers: one counter takes nearly 65535 hits per round), a slot whose longest read sets the
    rounds for reads half as long, a million poly-G heavy reads;
  - every k in 1..8 at lengths around the fused / unfused split and the tiers (5 .. 1000 bases);
  - byte edges: the reference's own answers for quality bytes below '!' or above '~', NUL runs (the all-NUL k-mer) and exotic
    bases (tests/golden/qc_edges.json.gz), through packed batches and FASTQ text, then a 50 k-pair scale-up against the oracle;
  - a million N-rich reads in the open-addressing table (at most half its capacity, checked before the launch)."""
import numpy as np
import pytest

from afterqc_amd import capi, synth
from oracle import oracle
from test_gpu_parity import default_cfg, run_both, assert_same
from test_gpu_spans import pad

import qc_compare

pytestmark = pytest.mark.gpu

KMER_CAP = 1 << 21          # the open-addressing table's capacity (aqc_ctx.hpp)
WORKERS = 4


def qc_both(gpu_engine, cfg, batches, whichs_pre=True, post=True, pieces=None):
    """the same qc_stat calls on the device and the oracle.  batches: [Batch] uploaded in turn (CLI pattern: first_index set by the
    caller); pieces: [(first, count)] per batch (default: one call for the whole batch)"""
    engines = (gpu_engine, oracle.OracleEngine())
    for eng in engines:
        eng.set_config(cfg)
        eng.reset_stats()
        for bi, b in enumerate(batches):
            slot = bi % 2
            eng.upload(slot, b)
            ranges = pieces or [(0, b.n)]
            mates = (0, 1) if cfg.paired else (0,)
            if whichs_pre:
                for first, count in ranges:
                    for m in mates:
                        eng.qc_stat(slot, capi.QC_R1_PRE if m == 0 else capi.QC_R2_PRE, m, first, count, 0)
            if post:
                eng.run(slot)
                for first, count in ranges:
                    for m in mates:
                        eng.qc_stat(slot, capi.QC_R1_POST if m == 0 else capi.QC_R2_POST, m, first, count, 1)
            eng.sync(slot)
    return engines


def whichs_of(cfg, pre=True, post=True):
    w = []
    if pre:
        w += [capi.QC_R1_PRE] + ([capi.QC_R2_PRE] if cfg.paired else [])
    if post:
        w += [capi.QC_R1_POST] + ([capi.QC_R2_POST] if cfg.paired else [])
    return w


def pairs_batch(d, lo=0, hi=None, first_index=0):
    hi = len(d["len1"]) if hi is None else hi
    return capi.Batch.from_matrices(d["seq1"][lo:hi], d["qual1"][lo:hi], d["len1"][lo:hi], d["seq2"][lo:hi], d["qual2"][lo:hi],
                                    d["len2"][lo:hi], first_index=first_index)


# ---- 1. the full sample -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def million_pairs():
    return synth.make_pairs(1_000_000, 150, seed=6061, dirty=True, workers=WORKERS)


def test_full_sample_one_call_per_object(gpu_engine, million_pairs):
    """1 M pairs, 2 x 150, config 3 dirty, k = 8: one aqc_qc_stat per object (> 512 * rpr_max reads: several k-mer launches)"""
    cfg = default_cfg(True)
    g, o = qc_both(gpu_engine, cfg, [pairs_batch(million_pairs)])
    qc_compare.assert_same_qc(g, o, whichs_of(cfg), 8, "1M one call")


def test_full_sample_cli_batches(gpu_engine, million_pairs):
    """the same pairs as the CLI feeds them: chunks of 131 072 records (global first_index), two slots in turn, k = 6"""
    cfg = default_cfg(True, qc_kmer=6)
    n, step = 1_000_000, 131_072
    batches = [pairs_batch(million_pairs, a, min(n, a + step), first_index=a) for a in range(0, n, step)]
    g, o = qc_both(gpu_engine, cfg, batches)
    qc_compare.assert_same_qc(g, o, whichs_of(cfg), 6, "1M chunked")


# ---- 2. slice saturation ------------------------------------------------------------------------------------------------------
def homopolymers(n_per, L, bases="ACGTN"):
    seqs, quals = [], []
    for c in bases:
        seqs += [c * L] * n_per
        quals += ["I" * L] * n_per
    return seqs, quals


@pytest.mark.parametrize("k", range(1, 9))
def test_homopolymer_rounds_saturate(gpu_engine, k):
    """reads of one repeated base at L = 150: one dense counter takes reads_per_round * (L - k) hits per round (65 462 of 65 535
    for k = 8); the counts must come out exact"""
    L, n_per = 150, 3000
    seqs, quals = homopolymers(n_per, L)
    batch = capi.Batch.from_strings(seqs, quals)
    cfg = default_cfg(False, qc_kmer=k)
    g, o = qc_both(gpu_engine, cfg, [batch], post=False)
    qc_compare.assert_same_qc(g, o, [capi.QC_R1_PRE], k, "homopolymer")
    got = dict(qc_compare.kmer_list(g.kmers(capi.QC_R1_PRE), k))
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    for c in "ACGTN":
        assert got[c * k] == n_per * (L - k)
        assert comp[c] * k in got
    assert len(got) == 5


def test_long_read_sets_the_rounds(gpu_engine):
    """one 288-base read among 150-base poly-G reads: the slot's max_len (cols 320: unfused) sizes the rounds for all of them"""
    seqs, quals = homopolymers(6000, 150, "G")
    seqs[3000] = "ACGT" * 72
    quals[3000] = "5" * 288
    batch = capi.Batch.from_strings(seqs, quals)
    for k in (3, 8):
        cfg = default_cfg(False, qc_kmer=k)
        g, o = qc_both(gpu_engine, cfg, [batch], post=False)
        qc_compare.assert_same_qc(g, o, [capi.QC_R1_PRE], k, "288 among 150")


def test_million_poly_g_heavy_reads(gpu_engine):
    """1 M single reads, half of them with poly-G runs of 40 .. 150 bases: the G counters saturate every round"""
    d = synth.make_single(1_000_000, 150, seed=6062, workers=WORKERS)
    rng = np.random.default_rng(6063)
    seq = d["seq1"]
    rows = np.nonzero(rng.random(len(seq)) < 0.5)[0]
    starts = rng.integers(0, 111, len(rows))
    cols = np.arange(150)[None, :]
    seq[rows] = np.where(cols >= starts[:, None], np.uint8(ord("G")), seq[rows])
    batch = capi.Batch.from_matrices(seq, d["qual1"], d["len1"])
    cfg = default_cfg(False)
    g, o = qc_both(gpu_engine, cfg, [batch])
    qc_compare.assert_same_qc(g, o, whichs_of(cfg), 8, "poly-G")


# ---- 3. k x length grid -------------------------------------------------------------------------------------------------------
def random_pairs(n, L, seed):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTN", dtype=np.uint8)
    qa = np.frombuffer(b"#+5?FIJ", dtype=np.uint8)
    mats = [alphabet[rng.integers(0, len(alphabet), (n, L))], qa[rng.integers(0, len(qa), (n, L))],
            alphabet[rng.integers(0, len(alphabet), (n, L))], qa[rng.integers(0, len(qa), (n, L))]]
    lens = np.full(n, L, dtype=np.uint32)
    return capi.Batch.from_matrices(mats[0], mats[1], lens, mats[2], mats[3], lens)


@pytest.mark.parametrize("L", [5, 8, 9, 100, 160, 161, 256, 257, 288, 289, 1000])
def test_k_by_length_grid(gpu_engine, L):
    """k = 1..8 at each length, pre and post: fused per-cycle rows up to 256 columns, qc_stat_kernel beyond"""
    batch = random_pairs(1500 if L <= 300 else 400, L, 7000 + L)
    for k in range(1, 9):
        cfg = default_cfg(True, qc_kmer=k, seq_len_req=1, n_base_limit=1000, unqualified_base_limit=0, poly_size_limit=0)
        g, o = qc_both(gpu_engine, cfg, [batch])
        qc_compare.assert_same_qc(g, o, whichs_of(cfg), k, "L=%d" % L)
        assert g.qc(capi.QC_R1_POST)[capi.QC_SCALARS, 1] > 0


# ---- 4. byte edges --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges():
    return qc_compare.load_edges()


def fastq_text(seqs, quals):
    return b"".join(b"@e%d\n%s\n+\n%s\n" % (i, s.encode("latin-1"), q.encode("latin-1")) for i, (s, q) in enumerate(zip(seqs, quals)))


def edges_on_device(eng, edges, k, how):
    seqs = [s for s, _ in edges["reads"]]
    quals = [q for _, q in edges["reads"]]
    eng.set_config(default_cfg(False, qc_kmer=k))
    eng.reset_stats()
    if how == "batch":
        eng.upload(0, capi.Batch.from_strings(seqs, quals))
        n = len(seqs)
    else:
        t = fastq_text(seqs, quals)
        info = eng.frame(0, pad(t), len(t), True)
        n = int(info.n)
        assert n == len(seqs)
    eng.qc_stat(0, capi.QC_R1_PRE, 0, 0, n, 0)
    return eng.qc(capi.QC_R1_PRE), eng.kmers(capi.QC_R1_PRE)


@pytest.mark.parametrize("how", ["batch", "text"])
@pytest.mark.parametrize("k", range(1, 9))
def test_edges_vs_reference(gpu_engine, edges, k, how):
    """the reference's statRead on quality bytes 0x00-0x20 / 0x7f-0xff inside the line, NUL runs, exotic bases, 5 / k / k+1 bases,
    as a packed batch and as FASTQ text through aqc_frame: every QC row, and every k-mer that was seen with its count (the
    all-NUL k-mer among them)"""
    acc, km = edges_on_device(gpu_engine, edges, k, how)
    st = edges["stat"][str(k)]
    qc_compare.assert_acc_equal(acc, qc_compare.fixture_acc(st, len(edges["reads"])), "%s k=%d" % (how, k))
    got = qc_compare.kmer_list(km, k)
    exp = [tuple(x) for x in st["kmers"]]
    assert sorted(x for x in got if x[1]) == sorted(x for x in exp if x[1])
    assert dict(got)["\x00" * k] == dict(exp)["\x00" * k] > 0


RC_GAP = pytest.mark.xfail(strict=True, reason="known deviation, DESIGN.md: reverse-complement entries of k-mers that entered the "
                                               "dictionary as a reverse complement (bytes outside the COMP table)")


@pytest.mark.parametrize("k", [1, 2, pytest.param(3, marks=RC_GAP), pytest.param(4, marks=RC_GAP), 5, 6, 7, 8])
def test_edges_kmer_dict_vs_reference(gpu_engine, edges, k):
    """the whole dictionary of the same reads: keys, counts, insertion rank and the top k-mers"""
    _, km = edges_on_device(gpu_engine, edges, k, "batch")
    exp = [tuple(x) for x in edges["stat"][str(k)]["kmers"]]
    qc_compare.assert_kmers_equal(qc_compare.kmer_list(km, k), exp, k, "batch")
    assert capi.top_kmers(km, k) == qc_compare.top_from_list(exp)


def test_framing_line_ends_vs_reference(gpu_engine, edges):
    """aqc_frame on lines that end in each byte 0x00-0x20: records and stripped lengths as the reference's Reader reads bytes"""
    eng = gpu_engine
    eng.set_config(default_cfg(False, qc_kmer=4))
    for case in edges["reader"]:
        c = bytes([case["byte"]])
        t = b"@r1\nACGTACGTAC" + c + b"\n+\nIIIIIIIIII" + c + b"\n@r2\nGATTACA\n+\nFFFFFFF\n"
        eng.reset_stats()
        info = eng.frame(0, pad(t), len(t), True)
        n = int(info.n)
        assert n == len(case["binary"]), case
        if n:
            eng.qc_stat(0, capi.QC_R1_PRE, 0, 0, n, 0)
            tn = eng.qc(capi.QC_R1_PRE)[capi.QC_TOTAL_NUM]
            exp = np.zeros_like(tn)
            for rec in case["binary"]:
                exp[:rec[1]] += 1
            assert np.array_equal(tn, exp), case


def test_byte_edges_scale_up(gpu_engine):
    """50 k pairs with ~1 % of quality bytes below '!' (not '\\n') and NUL runs of 8 .. 20 bases in ~1 % of reads: verdicts, QC
    rows and k-mers against the oracle, k = 8 and 3"""
    d = synth.make_pairs(50_000, 150, seed=6064, dirty=True)
    rng = np.random.default_rng(6065)
    low = np.array([b for b in range(0x21) if b != 0x0a], dtype=np.uint8)
    for m in ("1", "2"):
        q, s, ln = d["qual" + m], d["seq" + m], d["len" + m]
        hit = (rng.random(q.shape) < 0.01) & (np.arange(q.shape[1])[None, :] < (ln[:, None].astype(np.int64) - 1))
        q[hit] = low[rng.integers(0, len(low), int(hit.sum()))]
        for r in np.nonzero(rng.random(len(s)) < 0.01)[0]:
            run = int(rng.integers(8, 21))
            at = int(rng.integers(0, max(1, int(ln[r]) - run - 1)))
            s[r, at:at + run] = 0
    batch = pairs_batch(d)
    for k in (8, 3):
        # (no overlap walk: a NUL inside an overlap is a KeyError upstream, which ends the run)
        g, o = run_both(gpu_engine, default_cfg(True, qc_kmer=k, no_overlap=1), batch)
        # (a NUL is outside the COMP table: the dictionary's zero-count reverse-complement entries and ranks are the known deviation
        #  of DESIGN.md; verdicts, every QC row and every seen k-mer with its count must be exact)
        for r in (g, o):
            r["kmers"] = [sorted((kk, c) for kk, c in zip(*km) if c) for km in r["kmers"]]
        assert_same(g, o)
        nul = "\x00" * k
        got = dict(qc_compare.kmer_list(gpu_engine.kmers(capi.QC_R1_PRE), k))
        assert got.get(nul, 0) > 0


# ---- 5. exotic table load -----------------------------------------------------------------------------------------------------
def test_million_n_rich_reads_in_the_table(gpu_engine):
    """1 M single reads with 3 % N: the k-mers with anything but A/C/G/T (and their reverse complements)
    fill at most half of the open-addressing table — counted with numpy before the launch"""
    n, L, k = 1_000_000, 150, 8
    d = synth.make_single(n, L, seed=6066, workers=WORKERS)
    rng = np.random.default_rng(6067)
    seq = d["seq1"]
    seq[rng.random(seq.shape) < 0.03] = ord("N")
    # distinct exotic k-mers (byte keys, little-endian as on the device) + their reverse complements
    acgt = np.zeros(256, dtype=bool)
    acgt[list(b"ACGT")] = True
    comp = np.full(256, ord("N"), dtype=np.uint64)
    for a, b in (b"AT", b"TA", b"CG", b"GC", b"NN", b"at", b"ta", b"cg", b"gc"):
        comp[a] = b
    keys, rkeys = [], []
    for lo in range(0, n, 100_000):
        blk = seq[lo:lo + 100_000].astype(np.uint64)
        win = np.lib.stride_tricks.sliding_window_view(blk, k, axis=1)[:, :L - k]     # the L - k k-mers statRead takes
        bad = ~np.lib.stride_tricks.sliding_window_view(acgt[seq[lo:lo + 100_000]], k, axis=1)[:, :L - k].all(axis=2)
        w = win[bad]
        sh = (np.arange(k, dtype=np.uint64) * np.uint64(8))[None, :]
        keys.append(np.unique((w << sh).sum(axis=1, dtype=np.uint64)))
        rkeys.append(np.unique((comp[w[:, ::-1].astype(np.intp)] << sh).sum(axis=1, dtype=np.uint64)))
    distinct = len(np.unique(np.concatenate(keys + rkeys)))
    assert 50_000 < distinct <= KMER_CAP // 2, distinct
    batch = capi.Batch.from_matrices(seq, d["qual1"], d["len1"])
    cfg = default_cfg(False, n_base_limit=1000)
    g, o = qc_both(gpu_engine, cfg, [batch])
    qc_compare.assert_same_qc(g, o, whichs_of(cfg), k, "N-rich")
    keys_g = g.kmers(capi.QC_R1_PRE)[0]
    assert len(keys_g) >= distinct
