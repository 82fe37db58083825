"""-m gpu: the device's text writer (csrc/aqc_fmt.hpp, aqc_fmtcopy.hpp: the sizing pass, the tile bases, fmt_place_copy_kernel,
fmt_plan_kernel, fmt_plan_listed_kernel, the two whole-record copies, fmt_copy_kernel) at its window, piece, plan and list edges.
The inputs are those of tests/writer_cases.py — test_writer_cases_cpu.py shows on the CPU that they reach the shapes they are named
for — and every comparison is byte for byte against oracle.OracleEngine() (seqFilter.writeReads, preprocesser.py:206-232;
moveBarcodeToName, barcodeprocesser.py:34-45): verdict records first, then the six streams and their sizes, for format(), the
overlap store, format_spans() assembled the way the file writers do, the merged reads, and cuts at n, n - 1, 129 and 1 records."""
import json
import os
import subprocess
import sys

import pytest

import writer_cases as wc
from afterqc_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_small_own(gpu_engine, paired):
    """records of 8 .. 80 bytes at every source alignment: listed below 16 bytes, their own bytes from 16 on (one window up to 31)"""
    cfg, t1, t2, extra = wc.small_own(paired)
    res = wc.check(gpu_engine, cfg, t1, t2, ("plain", "spans"))
    wc.cover_small_own(cfg, t1, t2, res)
    # the expected output is the input itself
    sizes = gpu_engine.format(0, extra["n"], False)
    got = wc.fetch_streams(gpu_engine, 0, sizes)
    assert got[0] == t1 and (not paired or got[3] == t2) and sizes[1] == sizes[4] == 0


@pytest.mark.parametrize("mask,nocorr", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["fix", "fix_mask", "none", "mask"])
def test_patched_own(gpu_engine, mask, nocorr):
    """own-bytes records with up to four byte patches, five and six on the overflow path, patches in the end-aligned last window"""
    cfg, t1, t2, extra = wc.patched_own(mask, nocorr)
    res = wc.check(gpu_engine, cfg, t1, t2, ("plain", "overlap", "spans", "merged"))
    wc.cover_patched_own(cfg, t1, t2, res)


@pytest.mark.parametrize("paired,len_req", [(False, 0), (True, 0), (False, 16), (True, 16)], ids=["se", "pe", "se_len_req", "pe_len_req"])
def test_piece_lengths(gpu_engine, paired, len_req):
    """trimmed records: bases and quality pieces of 1 .. 17, 30 .. 34, 46 .. 50, 62 .. 66 bytes at every alignment, flag literals"""
    cfg, t1, t2, extra = wc.piece_lengths(paired, len_req)
    res = wc.check(gpu_engine, cfg, t1, t2, ("plain", "spans"))
    wc.cover_piece_lengths(cfg, t1, t2, res)


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_barcode_names(gpu_engine, paired):
    """the barcode writer (the dense-plan kernel alone, find_colon, the moved-barcode piece) on names of every shape"""
    cfg, t1, t2, extra = wc.barcode_names(paired)
    res = wc.check(gpu_engine, cfg, t1, t2, ("plain", "overlap") if paired else ("plain",))
    wc.cover_barcode_names(cfg, t1, t2, res, extra["classes"])


@pytest.mark.parametrize("last", ["complete", "no_newline", "blanks"])
@pytest.mark.parametrize("barcode", [0, 1], ids=["plain_names", "barcode"])
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_stripped_line_ends(gpu_engine, paired, barcode, last):
    """newlines that are literal pieces: 8, 9 and 10 pieces per record, the last being FMT_MAXP"""
    cfg, t1, t2, extra = wc.stripped_line_ends(paired, barcode, last)
    res = wc.check(gpu_engine, cfg, t1, t2, ("plain", "spans"))
    wc.cover_stripped_line_ends(cfg, t1, t2, res)


@pytest.mark.parametrize("trim_tail", [0, 1], ids=["untrimmed", "trim_tail"])
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_long_records(gpu_engine, paired, trim_tail):
    """records over 512 bytes (listed), pieces of up to 1000 bytes, 64 against 65 work items, a 600-byte name"""
    cfg, t1, t2, extra = wc.long_records(paired, trim_tail)
    res = wc.check(gpu_engine, cfg, t1, t2, ("plain",))
    wc.cover_long_records(cfg, t1, t2, res)


@pytest.mark.parametrize("store", [False, True], ids=["plain", "overlap_store"])
def test_index_records(gpu_engine, store):
    """aqc_format_plain: whole index records of 8 .. 80 and 470 .. 540 bytes, routed and renamed by the verdicts of a pair run"""
    from oracle import oracle
    cfg, t1, t2, extra = wc.index_verdict_run(store)
    n = extra["n"]
    i1, i2 = wc.index_records(n)
    ora = oracle.OracleEngine()
    streams = []
    for eng in (gpu_engine, ora):
        info, n_run, res = wc.frame_run(eng, cfg, t1, t2, slot=0)
        assert n_run == n
        finfo = eng.frame(1, wc.pad(i1), len(i1), True, wc.pad(i2), len(i2), True)
        assert int(finfo.n) == n
        out = []
        for cut in (n, n - 1, 129, 1):
            sizes = eng.format_plain(1, 0, cut, store)
            out.append((sizes, wc.fetch_streams(eng, 1, sizes)))
        streams.append((res, out))
    ora.close()
    gpu_engine.reset_stats()
    (res_g, out_g), (res_o, out_o) = streams
    assert res_g.tobytes() == res_o.tobytes()
    flags = res_o["flag"]
    assert (flags == capi.GOOD).sum() >= 100 and (store or (flags != capi.GOOD).sum() >= 100)
    for (sg, g), (so, o) in zip(out_g, out_o):
        wc.assert_streams(sg, g, so, o, "format_plain")
    if store:
        assert out_o[0][0][2] > 0 and out_o[0][0][5] > 0          # (the overlap streams hold whole index records)


def test_many_tiles_share_the_general_lists(gpu_engine):
    """257 tiles, every record listed: tile 256 appends to the list tile 0 filled"""
    cfg, t1, _, extra = wc.many_tiles_a()
    wc.check_expected(gpu_engine, cfg, t1, None, extra["expected"], extra["n"])


def test_many_tiles_second_round_of_the_base_scan():
    """more than TXT_BLOCK x 8 super-tiles: fmt_tile_bases_kernel carries both streams' bytes into its second round (in a context of
    its own: its buffers are sized for two million records)"""
    cfg, t1, _, extra = wc.many_tiles_b()
    eng = capi.Engine(0, 1)
    try:
        wc.check_expected(eng, cfg, t1, None, extra["expected"], extra["n"])
    finally:
        eng.close()


# ---- the plan / whole-copy pair of kernels in place of place + copy: AQC_PLACE_COPY=0, read once per process ----------------------------
def child_plan_whole():
    eng = capi.Engine(0, 1)
    done = []
    for name, (cfg, t1, t2, extra), modes in (("small_own", wc.small_own(True), ("plain",)),
                                              ("patched_own", wc.patched_own(1, 0), ("plain", "overlap")),
                                              ("piece_lengths", wc.piece_lengths(True), ("plain",))):
        wc.check(eng, cfg, t1, t2, modes)
        done.append(name)
    eng.close()
    print(json.dumps({"place_copy": os.environ.get("AQC_PLACE_COPY"), "checked": done}))


def test_plan_and_whole_copy_kernels_in_a_child_process():
    """fmt_plan_kernel + fmt_copy_whole_kernel as the main pass's writer (a fresh process: it replaces none that has the GPU open)"""
    env = dict(os.environ, AQC_PLACE_COPY="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "plan_whole"], capture_output=True, text=True, timeout=300, env=env, cwd=os.path.join(ROOT, "tests"))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == {"place_copy": "0", "checked": ["small_own", "patched_own", "piece_lengths"]}


if __name__ == "__main__":
    {"plan_whole": child_plan_whole}[sys.argv[1]]()
