"""Shared by the QC edge / scale tests: the qc_edges fixture as engine-shaped data, and full comparisons of QC rows and k-mer
dictionaries (keys, counts, insertion rank, top k-mers) between two engines or an engine and the fixture."""
import gzip
import json
import os

import numpy as np

from afterqc_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_edges():
    with gzip.open(os.path.join(GOLDEN, "qc_edges.json.gz"), "rt") as f:
        return json.load(f)


def fixture_acc(st, n_reads):
    """one statRead capture of the fixture -> the [QC_ROWS, AQC_QC_COLS] accumulator layout of aqc_get_qc"""
    a = np.zeros((capi.QC_ROWS, capi.AQC_QC_COLS), dtype=np.int64)
    n = len(st["total_num"])
    a[capi.QC_TOTAL_NUM, :n] = st["total_num"]
    a[capi.QC_TOTAL_QUAL, :n] = st["total_qual"]
    for i, b in enumerate("ATCG"):
        a[capi.QC_BASE_COUNT_A + i, :n] = st["base_count"][b]
        a[capi.QC_BASE_QUAL_A + i, :n] = st["base_qual"][b]
    a[capi.QC_DISCONTINUITY, :n] = st["discontinuity"]
    a[capi.QC_GC_HIST, :len(st["gc_hist"])] = st["gc_hist"]
    a[capi.QC_SCALARS, 0] = st["total_kmer"]
    a[capi.QC_SCALARS, 1] = n_reads
    return a


def kmer_list(kmers, k):
    """(keys, counts, order) of an engine -> [(k-mer as latin-1 text, count)] in dict insertion order"""
    keys, counts, order = kmers
    idx = np.argsort(np.asarray(order, dtype=np.uint64), kind="stable")
    return [(int(keys[i]).to_bytes(8, "little")[:k].decode("latin-1"), int(counts[i])) for i in idx]


ROW_NAMES = ["TOTAL_NUM", "TOTAL_QUAL", "COUNT_A", "COUNT_T", "COUNT_C", "COUNT_G", "QUAL_A", "QUAL_T", "QUAL_C", "QUAL_G",
             "DISCONTINUITY", "GC_HIST", "SCALARS"]


def assert_acc_equal(got, exp, what=""):
    got, exp = np.asarray(got), np.asarray(exp)
    if np.array_equal(got, exp):
        return
    r, c = np.argwhere(got != exp)[0]
    raise AssertionError("%s QC row %s col %d: got %d, expected %d (%d cells differ)"
                         % (what, ROW_NAMES[r], c, got[r, c], exp[r, c], int((got != exp).sum())))


def assert_kmers_equal(got, exp, k, what=""):
    """got / exp: [(k-mer, count)] in insertion order; also the top-10 list of the report"""
    if got == exp:
        return
    dg, de = dict(got), dict(exp)
    missing = [km for km in de if km not in dg]
    extra = [km for km in dg if km not in de]
    wrong = [(km, dg[km], de[km]) for km in de if km in dg and dg[km] != de[km]]
    first = next(i for i in range(min(len(got), len(exp)) + 1) if i >= min(len(got), len(exp)) or got[i] != exp[i])
    raise AssertionError("%s k=%d k-mer dict differs: %d vs %d entries, missing %r, extra %r, counts %r, first rank difference at %d"
                         % (what, k, len(got), len(exp), missing[:5], extra[:5], wrong[:5], first))


def top_from_list(items, top=10):
    """sortKmer (qualitycontrol.py:155-156) on an insertion-ordered list: count descending, insertion order for ties"""
    return [[km, c] for km, c in sorted(items, key=lambda x: -x[1])[:top]]


def assert_same_qc(eng_a, eng_b, whichs, k, what=""):
    """every QC row and the whole k-mer dictionary of two engines (device vs oracle), plus capi.top_kmers"""
    for w in whichs:
        assert_acc_equal(eng_a.qc(w), eng_b.qc(w), "%s which=%d" % (what, w))
        ka, kb = eng_a.kmers(w), eng_b.kmers(w)
        la, lb = kmer_list(ka, k), kmer_list(kb, k)
        assert_kmers_equal(la, lb, k, "%s which=%d" % (what, w))
        assert capi.top_kmers(ka, k) == capi.top_kmers(kb, k) == top_from_list(lb)
