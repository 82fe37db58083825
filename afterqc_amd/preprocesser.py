"""Per-file driver: the batch-pipelined counterpart of the reference's seqFilter
(preprocesser.py:141-783).  Same constructor / run() interface and the same outputs
(good/bad/overlap FASTQ, QC/<R1 basename>.json), but the per-read loop of preprocesser.py:411-631
is not executed here: records are framed in bulk (afterqc_amd.fastq), shipped to the GPU as SoA
batches, judged by the HIP kernels behind the C ABI (afterqc_amd.capi.Engine) and only the 32-byte
verdict records come back.  This module is I/O and bookkeeping:

  pass 1  pre-filter QC sampling + auto-trim            (preprocesser.py:247-280)
  pass 2  every run takes the text path: raw text chunk -> aqc_frame -> aqc_run -> aqc_qc_stat(post) -> aqc_format ->
          good / bad / overlap text back -> files; framing and formatting happen on the device.
            * whole-input pipe (aqc_pipe_run, C++ reader / slot-worker / writer threads; the default for read files
              without index files and without --qc_only): chunks of exactly `chunk_records` records, dealt round robin
              over every engine (= GPU) the filter was given, outputs stitched in chunk order, statistics summed on
              the host;
            * serial chunk loop in this file (_run_text / _run_text_indexed): index files, --qc_only, inputs of
              irregular shape (the pipe reports them), injected engines;
          the host path (_run_host: numpy framing, Python writer) only exists as a cross-check (use_text_path=False);
          the three serial drivers state upstream's loop rules once: lock_step (which reader ends the loop) and
          seqFilter._judge (the loop body: --qc_only, the post-filter sampling window, death at a record)
  stats   counters -> JSON with the reference's schema  (preprocesser.py:660-778)

There is no CPU compute path: `engine` defaults to the HIP engine, which raises if the library or
the GPU is missing.  (Tests inject the oracle engine to exercise THIS file's host logic on CPU.)
"""
import json
import os
import sys
import queue
import threading
import time

import numpy as np

from . import adapter_detect, capi, fastq
from .qc import QualityControl, ALL_BASES

FLAG_BYTES = [b"", b"BADBCD1", b"BADBCD2", b"BADTRIM1", b"BADTRIM2", b"BADBBL", b"BADLEN", b"BADPOL", b"BADLQC",
              b"BADNCT", b"BADDIFF", b"BADMISMATCH"]


def getMainName(filename):
    """preprocesser.py:14-17"""
    base = os.path.basename(filename)
    for ext in (".fastq", ".fq", ".gz"):
        base = base.replace(ext, "")
    return base


# the keys echoed into the JSON "command" block (makeDict, preprocesser.py:86-123)
COMMAND_KEYS = ("index2_flag", "draw", "barcode", "index1_flag", "seq_len_req", "index1_file",
                "overlap_output_folder", "trim_tail", "trim_pair_same", "poly_size_limit", "good_output_folder",
                "debubble_dir", "index2_file", "qualified_quality_phred", "barcode_flag", "trim_front",
                "barcode_verify", "read2_file", "n_base_limit", "barcode_length", "trim_tail2",
                "unqualified_base_limit", "allow_mismatch_in_poly", "input_dir", "read1_file", "read2_flag",
                "store_overlap", "debubble", "read1_flag", "trim_front2", "bad_output_folder", "qc_only", "qc_sample",
                "qc_kmer")


def input_files(opt):
    return [opt.read1_file, opt.read2_file, opt.index1_file, opt.index2_file]


def third_stream_mode(opt, paired):
    """What the writers' third stream per file holds (capi.STORE_*): nothing, the overlap tails of --store_overlap, or — pairs
    only — the merged reads of --store_merged (after.finalize_options refuses the two together)."""
    if getattr(opt, "store_merged", False):
        return capi.STORE_MERGED if paired else capi.STORE_OFF
    return capi.STORE_OVERLAP if opt.store_overlap else capi.STORE_OFF


def merged_record(name1, s1, p1, q1, s2, q2, ov):
    """The merged read of a pair whose mates go to the good files as (name1, s1, p1, q1) and (.., s2, .., q2) with overlap_len
    `ov`: read 1, then the part of read 2 outside the overlap — reverse complement (util.reverseComplement: COMP, anything
    else 'N') and reversed qualities.  None: a mate's quality line is not as long as its sequence line, no merged read."""
    if len(q1) != len(s1) or len(q2) != len(s2):
        return None
    p = len(s2) - ov
    return (name1 + b"\n" + bytes(s1) + bytes(s2[0:p]).translate(REVCOMP_TABLE)[::-1] + b"\n" + p1 + b"\n"
            + bytes(q1) + bytes(q2[0:p])[::-1] + b"\n")


REVCOMP_TABLE = bytes(b"TGCAtgcaN"[b"ACGTacgtN".index(bytes([c]))] if bytes([c]) in b"ACGTacgtN" else ord("N") for c in range(256))


def makeDict(opt):
    return {k: getattr(opt, k) for k in COMMAND_KEYS}


def load_circles(debubble_dir):
    """loadBubbleCircles (preprocesser.py:157-174): rows of x,y,radius,lane,tile after a header line."""
    path = os.path.join(debubble_dir, "circles.csv")
    circles = []
    if not os.path.exists(path):
        return circles
    with open(path) as f:
        for row in f.readlines()[1:]:
            r = row.split(",")
            circles.append((float(r[0]), float(r[1]), float(r[2]), int(r[3]), int(r[4])))
    return circles


def cut_config(opt):
    """--cut_front / --cut_tail / --cut_right as the engine takes them; None: every mode is off (options objects built without
    the cut options count as off)"""
    modes = [bool(getattr(opt, k, False)) for k in ("cut_front", "cut_tail", "cut_right")]
    if not any(modes):
        return None
    return capi.CutConfig(int(modes[0]), int(modes[1]), int(modes[2]), int(getattr(opt, "cut_window_size", 4)), int(getattr(opt, "cut_mean_quality", 20)))


def adapter_auto(opt):
    """which mates' adapters are to be found in the pass-1 sample (--adapter_sequence auto / --adapter_sequence_r2 auto) -> (read 1,
    read 2); single-end input has no read 2"""
    a1, a2 = (adapter_detect.is_auto(getattr(opt, k, None)) for k in ("adapter_sequence", "adapter_sequence_r2"))
    return a1, a2 and getattr(opt, "read2_file", None) is not None


def adapter_config(opt, found=("", "")):
    """--adapter_sequence / --adapter_sequence_r2 / --adapter_min_overlap as the engine takes them; None: no adapter is given
    (options objects built without the adapter options count as off).  Single-end input has no read 2 to search.  A mate whose
    option says `auto` takes what was found for it; nothing found, or nothing looked for yet: it is not searched."""
    given = [getattr(opt, k, None) or "" for k in ("adapter_sequence", "adapter_sequence_r2")]
    a1, a2 = (f if adapter_detect.is_auto(a) else a for a, f in zip(given, found))
    if getattr(opt, "read2_file", None) is None:
        a2 = ""
    if not a1 and not a2:
        return None
    return capi.AdapterConfig(a1, a2, int(getattr(opt, "adapter_min_overlap", 4)))


def poly_config(opt):
    """--trim_poly_g / --trim_poly_x and their minimum lengths as the engine takes them; None: both are off (options objects built
    without the poly options count as off).  --trim_poly_x tries A, C, G and T; with both on, G takes the smaller length."""
    on_g, on_x = bool(getattr(opt, "trim_poly_g", False)), bool(getattr(opt, "trim_poly_x", False))
    if not on_g and not on_x:
        return None
    lg = int(getattr(opt, "poly_g_min_len", 10)) if on_g else 0
    lx = int(getattr(opt, "poly_x_min_len", 10)) if on_x else 0
    return capi.PolyConfig(lx, lx, min(lg, lx) if on_g and on_x else lg or lx, lx)


# the passes in front of the verdict kernel that an option switches on: the engine's setter, the options it stands for
VIEW_PASSES = (("set_quality_cut", "--cut_front / --cut_tail / --cut_right"),
               ("set_adapter_trim", "--adapter_sequence / --adapter_sequence_r2"),
               ("set_poly_trim", "--trim_poly_g / --trim_poly_x"))


def set_view_passes(engine, configs, clear=False):
    """the quality cut, the adapters and the poly tails (configs: one per entry of VIEW_PASSES, None: off) on an engine.  A pass that is on needs
    an engine that has it: an error, never a run without the option.  clear: a pass that is off is switched off on an engine that
    has it (an engine the caller handed over may come from a run that had it on)"""
    for (setter, options), config in zip(VIEW_PASSES, configs):
        if config is not None and not hasattr(engine, setter):
            raise RuntimeError("afterqc_amd: %s need an engine with %s; %s has none" % (options, setter, type(engine).__name__))
        if config is not None or (clear and hasattr(engine, setter)):
            getattr(engine, setter)(config)


def build_config(opt, paired, has_index2):
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.count_r2_bases = 1 if has_index2 else 0
    cfg.trim_front, cfg.trim_tail = max(opt.trim_front, 0), max(opt.trim_tail, 0)
    cfg.trim_front2, cfg.trim_tail2 = max(opt.trim_front2, 0), max(opt.trim_tail2, 0)
    cfg.seq_len_req = opt.seq_len_req
    cfg.poly_size_limit = opt.poly_size_limit
    cfg.allow_mismatch_in_poly = opt.allow_mismatch_in_poly
    cfg.qualified_quality_phred = opt.qualified_quality_phred
    cfg.unqualified_base_limit = opt.unqualified_base_limit
    cfg.n_base_limit = opt.n_base_limit
    cfg.no_overlap = 1 if opt.no_overlap else 0
    cfg.no_correction = 1 if opt.no_correction else 0
    cfg.mask_mismatch = 1 if opt.mask_mismatch else 0
    cfg.barcode = 1 if opt.barcode else 0
    cfg.barcode_length = opt.barcode_length
    cfg.set_verify(opt.barcode_verify)
    cfg.debubble = 1 if opt.debubble else 0
    cfg.qc_kmer = opt.qc_kmer
    return cfg


class _Outputs:
    """The good / bad / overlap writers of preprocesser.py:323-371 for up to four input files, opened at the paths
    seqFilter._layout gives (None: not written; a gzip output carries its .gz in the name, which fastq.Writer goes by)."""

    def __init__(self, paths, gzip_comp):
        opened = [[None if p is None else fastq.Writer(p, False, gzip_comp) for p in per_file] for per_file in paths]
        self.good, self.bad, self.overlap = ([w[q] for w in opened] for q in range(3))
        self.per_file = [tuple(w) for w in opened]

    def close(self):
        for group in (self.good, self.bad, self.overlap):
            for w in group:
                if w is not None:
                    w.close()


class _TextInput:
    """One input file as a stream of raw text chunks in two page-locked buffers.  A side thread reads the file into
    the buffer the main loop is not using; the unconsumed tail of a chunk is carried to the front of the next."""

    def __init__(self, eng, fname, chunk_bytes):
        self.eng = eng
        self.f = fastq.open_binary(fname)
        self.cap = max(int(chunk_bytes), 256)
        self.bufs = [eng.host_buffer(self.cap), eng.host_buffer(self.cap)]
        self.req = queue.Queue()
        self.done = queue.Queue()
        self.file_eof = False
        self.thread = threading.Thread(target=self._reader, daemon=True)
        self.thread.start()

    def _reader(self):
        while True:
            job = self.req.get()
            if job is None:
                return
            which, off = job
            try:
                view = self.bufs[which].view
                end = off
                final = self.file_eof
                while not final and end < self.cap:
                    got = self.f.readinto(view[end:self.cap])
                    if not got:
                        final = self.file_eof = True
                    else:
                        end += got
                self.done.put((end, final))
            except BaseException as e:      # surfaced by wait_fill on the main thread
                self.done.put(e)

    def start_fill(self, which, off):
        self.req.put((which, off))

    def wait_fill(self):
        r = self.done.get()
        if isinstance(r, BaseException):
            raise r
        return r

    def grow(self, which):
        """double both buffers (a single record did not fit)"""
        ncap = self.cap * 2
        nb = [self.eng.host_buffer(ncap), self.eng.host_buffer(ncap)]
        nb[which].array[:self.cap] = self.bufs[which].array[:self.cap]
        for b in self.bufs:
            b.free()
        self.bufs, self.cap = nb, ncap

    def carry(self, cur, consumed, nbytes, final, finished):
        """tail of buffer `cur` -> head of the other buffer, then ask the reader for the rest of it.
        `finished`: an empty line ended this file (fastq.py:44-47): nothing after it is ever read"""
        nxt = 1 - cur
        if finished:
            self.file_eof = True
            self.done.put((0, True))
            return
        left = nbytes - consumed
        if left:
            self.bufs[nxt].array[:left] = self.bufs[cur].array[consumed:nbytes]
        if final:
            self.done.put((left, True))
        else:
            self.start_fill(nxt, left)

    def close(self):
        self.req.put(None)
        self.thread.join()
        self.f.close()
        for b in self.bufs:
            b.free()


class _TextSink:
    """The good / bad writers of every file fed from the device.  The main loop only queues (slot, sizes) after
    aqc_format; a fetch thread copies the four formatted streams of that slot into page-locked buffers (and then
    releases the slot for the next chunk), a write thread writes them in order.  With two slots the upload and
    kernels of chunk i+1 overlap the download and file writes of chunk i."""

    N_SETS = 3

    def __init__(self, eng, writers, n_slots, store_overlap=False):
        self.eng = eng
        self.store_overlap = store_overlap
        self.writers = writers                       # per file (good, bad, overlap); None = not written
        self.sets = [[None] * 6 for _ in range(self.N_SETS)]
        self.set_free = [threading.Semaphore(1) for _ in range(self.N_SETS)]
        self.slot_free = [threading.Semaphore(1) for _ in range(n_slots)]
        self.fq = queue.Queue()
        self.wq = queue.Queue()
        self.err = None
        self.death = None                            # upstream's run ends inside a chunk (death_record): raised once all is written
        self.dead = False
        self.fetcher = threading.Thread(target=self._fetch, daemon=True)
        self.writer = threading.Thread(target=self._write, daemon=True)
        self.fetcher.start()
        self.writer.start()

    def _fetch(self):
        which = 0
        while True:
            job = self.fq.get()
            if job is None:
                self.wq.put(None)
                return
            slot, sizes = job[0], job[1]
            died = len(job) > 2 and job[2]           # (the main loop cut this chunk at the record upstream dies at)

            def fetch_all(sizes):
                for q, nbytes in enumerate(sizes):
                    if q // 3 < len(self.writers) and nbytes and self.writers[q // 3][q % 3] is not None:
                        fetch_stream(self.eng, slot, q, nbytes, self.sets[which])

            try:
                self.set_free[which].acquire()           # the writer is done with this buffer set
                if self.err is None:
                    try:
                        fetch_all(sizes)
                    except capi.AqcError as e:
                        # an exception inside upstream's loop: its run ends at that record, what came before is written
                        k = death_record(self.eng, slot, e)
                        if k is None:
                            raise
                        sizes = self.eng.format(slot, k, self.store_overlap)
                        fetch_all(sizes)
                        self.death = e
                        died = True
            except BaseException as e:
                self.err = e
            finally:
                self.slot_free[slot].release()           # the slot may take the next chunk
                self.wq.put((which, list(sizes), died))
                which = (which + 1) % self.N_SETS

    def _write(self):
        while True:
            job = self.wq.get()
            if job is None:
                return
            which, sizes, died = job
            try:
                if self.err is None and not self.dead:
                    if died:
                        self.dead = True                 # this chunk is the last one written
                    for q, nbytes in enumerate(sizes):
                        if nbytes and q // 3 < len(self.writers) and self.writers[q // 3][q % 3] is not None:
                            self.writers[q // 3][q % 3].write_bytes(self.sets[which][q].view[:nbytes])
            except BaseException as e:
                self.err = e
            finally:
                self.set_free[which].release()

    def acquire_slot(self, slot):
        """block until the previous chunk of this slot has been fetched"""
        self.slot_free[slot].acquire()
        if self.err is not None:
            self.slot_free[slot].release()
            raise self.err

    def release_slot(self, slot):
        self.slot_free[slot].release()

    def emit(self, slot, sizes, death=None):
        if death is not None:
            self.death = death
        self.fq.put((slot, list(sizes), death is not None))

    def close(self):
        self.fq.put(None)
        self.fetcher.join()
        self.writer.join()
        for st in self.sets:
            for b in st:
                if b is not None:
                    b.free()
        if self.err is not None:
            raise self.err
        if self.death is not None:
            raise self.death


def death_record(eng, slot, e):
    """An exception INSIDE the reference's loop (KeyError / IndexError of the overlap walk, int() of a name field) ends its run
    at that record, with everything before it written.  -> the index of that record in the slot, or None when the error is
    not of that kind."""
    if isinstance(e, capi.AqcError) and e.code in capi.RECORD_ERRORS and hasattr(eng, "error_record"):
        return eng.error_record(slot)
    return None


def fetch_stream(eng, slot, q, nbytes, bufs):
    """stream q (= file * 3 + stream) of the slot's formatted text -> the page-locked buffer bufs[q], which grows to take it"""
    buf = bufs[q]
    if buf is None or buf.nbytes < nbytes:
        if buf is not None:
            buf.free()
        buf = bufs[q] = eng.host_buffer(nbytes + nbytes // 4 + 4096)
    eng.fetch_text(slot, q // 3, q % 3, buf.array, buf.nbytes)
    return buf


def frame_inputs(eng, slot, inputs, fills, cur, first_index, cap=capi.UINT64_MAX):
    """aqc_frame over buffer `cur` of one or two lock-stepped inputs (fills: per input (bytes in the buffer, the file ends
    there)) -> (info, per input (records available, an empty line ended the file (fastq.py:44-47), the file ends in this
    buffer, bytes consumed, bytes in the buffer))"""
    args = []
    for inp, (nbytes, final) in zip(inputs, fills):
        args += [inp.bufs[cur].array, nbytes, final]
    info = eng.frame(slot, *args, max_records=cap, first_index=first_index)
    framed = [(int(info.avail1), bool(info.eof1), int(info.consumed1)), (int(info.avail2), bool(info.eof2), int(info.consumed2))]
    return info, [(avail, eof, final, consumed, nbytes) for (avail, eof, consumed), (nbytes, final) in zip(framed, fills)]


def lock_step(state, info):
    """The reference reads one record of every input per turn, R1 first, and the first reader that returns None ends the
    loop (preprocesser.py:412-429).  state: per input, R1 first, frame_inputs' (avail, eof_seen, final_fill, ...); info: the
    reads' frame info — n, the records this chunk gives every input, and next_len1, the length of R1's record n.
    -> (stop, extra_bases, per input: nothing after this chunk is ever read from it)"""
    n = int(info.n)
    done = [(eof or final) and avail == n for avail, eof, final, *_ in state]
    if done[0]:
        return True, 0, done
    if any(done[1:]) and state[0][0] > n:
        # R1's next record was read (and counted into TOTAL_BASES, :416) before another reader ran dry
        return True, int(info.next_len1), done
    return False, 0, [s[1] or (k != 0 and done[k]) for k, s in enumerate(state)]


def advance(inputs, cur, n, state, finished):
    """every input goes on to its next chunk: what framing left of buffer `cur` is carried to the front of the other one"""
    for inp, (avail, eof, final, consumed, nbytes), fin in zip(inputs, state, finished):
        if n == 0 and not final and not eof and avail == 0:
            inp.grow(cur)                                  # not even one record fits the buffer
        inp.carry(cur, consumed, nbytes, final, fin)


class seqFilter:
    """seqFilter(options).run() — preprocesser.py:141-155,234-783."""

    def __init__(self, opt, engine=None, batch_records=1 << 20, device=0, chunk_bytes=64 << 20, use_text_path=True,
                 devices=None, use_pipe=True, chunk_records=1 << 17, pipe_slots=3, io_threads=0):
        self.options = opt
        self.chunk_bytes = chunk_bytes
        self.use_text_path = use_text_path
        self.text_path = False
        self.engine = engine
        self.device = device
        # devices: the GPUs one input is dealt over (default: just `device`); engines[0] is self.engine
        self.devices = list(devices) if devices else [device]
        self.extra_engines = []
        self.use_pipe = use_pipe
        self.used_pipe = False
        self.chunk_records = int(chunk_records)
        self.pipe_slots = int(pipe_slots)
        self.io_threads = int(io_threads)
        self.own_engine = False
        self.batch_records = max(int(batch_records), 1000)
        self.paired = opt.read2_file is not None
        self.bubbleCircles = []
        self.stat = None
        self.cut = cut_config(opt)
        self.adapter = adapter_config(opt)           # (a mate that says `auto` is not searched until run() has looked at the sample)
        self.adapter_auto = adapter_auto(opt)
        self.adapter_detect = None                   # what the census found, as the statistics JSON says it
        self.poly = poly_config(opt)

    # ---- helpers ---------------------------------------------------------------------------------
    def _engine(self):
        if self.engine is None:
            self.engine = capi.Engine(self.devices[0], max(2, self.pipe_slots))
            self.own_engine = True
        return self.engine

    def _engines(self, all_devices=False):
        """engines[0] is the run's engine; the contexts on the other devices are only created once the whole-input pipe has
        been chosen (all_devices=True) — a run that stays on one engine (index files, --qc_only, .bz2, the serial fallback)
        never touches another GPU"""
        eng = self._engine()
        if all_devices and self.own_engine and not self.extra_engines and len(self.devices) > 1:
            cfg, circles = self._last_cfg
            for d in self.devices[1:]:
                e = capi.Engine(d, max(2, self.pipe_slots))
                e.set_config(cfg)
                e.set_circles(circles)
                set_view_passes(e, (self.cut, self.adapter, self.poly))
                e.reset_stats()
                self.extra_engines.append(e)
        return [eng] + self.extra_engines

    def _aux(self, batch, rb1):
        """Parse lane/tile/x/y out of the R1 names for the bubble filter (preprocesser.py:180-192)."""
        n = rb1.n
        ok = np.zeros(n, np.uint8); lane = np.zeros(n, np.int32); tile = np.zeros(n, np.int32)
        x = np.zeros(n, np.int32); y = np.zeros(n, np.int32)
        for i in range(n):
            ok[i], lane[i], tile[i], x[i], y[i] = fastq.parse_illumina_name(rb1.line("name", i))
        batch.set_aux(lane, tile, x, y, ok)

    # ---- the run -----------------------------------------------------------------------------------
    def run(self):
        opt = self.options
        if opt.barcode and self.cut is not None:
            # (the barcode stage moves the view before the trim stage: that combination is not implemented; refused before anything is created)
            raise SystemExit("afterqc_amd: --cut_front / --cut_tail / --cut_right are not implemented for barcoded input "
                             "(%s); run it with --barcode off or without the cut" % opt.read1_file)
        if not self.paired and not getattr(opt, "adapter_sequence", None) and getattr(opt, "adapter_sequence_r2", None):
            # (never a silent run without the option: only read 2's adapter is given and this input has no read 2)
            raise SystemExit("afterqc_amd: --adapter_sequence_r2 is given alone but %s is single-end: there is no read 2 to search; "
                             "give the adapter as --adapter_sequence" % opt.read1_file)
        if opt.barcode and (self.adapter is not None or any(self.adapter_auto)):
            raise SystemExit("afterqc_amd: --adapter_sequence / --adapter_sequence_r2 are not implemented for barcoded input "
                             "(%s); run it with --barcode off or without the adapter" % opt.read1_file)
        if opt.barcode and self.poly is not None:
            raise SystemExit("afterqc_amd: --trim_poly_g / --trim_poly_x are not implemented for barcoded input "
                             "(%s); run it with --barcode off or without the poly-tail cut" % opt.read1_file)
        t_init = time.perf_counter()
        eng = self._engine()
        self.timing = {"init_s": time.perf_counter() - t_init}       # (a fresh process: HIP runtime start + the library's code object)
        t_run = time.perf_counter()
        if opt.debubble:
            self.bubbleCircles = load_circles(opt.debubble_dir)
        # no front trim if the sequence is barcoded (preprocesser.py:242-243)
        if opt.barcode:
            opt.trim_front = 0
        self._configure(first=True)
        r1pre, r2pre = self._sample(eng)
        self.timing["pass1_s"] = time.perf_counter() - t_run
        self._auto_trim(r1pre, r2pre)
        self._detect_adapters(eng)
        print(opt.read1_file + " options:")
        print(opt)
        qc_dir, gzip_out, paths = self._layout()
        self._configure()                            # the per-read settings now include the resolved trim values
        t_p2 = time.perf_counter()
        cpu_p2 = sum(os.times()[:2])
        extra_bases = self._pass2(eng, paths, gzip_out)
        self.timing["pass2_s"] = time.perf_counter() - t_p2
        self.timing["pass2_cpu_s"] = sum(os.times()[:2]) - cpu_p2          # user + system, all threads: how many cores pass 2 kept busy
        try:
            self._report(eng, r1pre, r2pre, extra_bases, qc_dir)
            self.timing["total_s"] = time.perf_counter() - t_run
        finally:
            t_close = time.perf_counter()
            if self.own_engine:
                for e in [self.engine] + self.extra_engines:
                    if e is not None:
                        e.close()
                self.engine = None
                self.extra_engines = []
            self.timing["close_s"] = time.perf_counter() - t_close
        return self.stat

    def _configure(self, first=False):
        """the options as they stand -> every engine of the run; first: the bubble circles too, and the statistics start at zero"""
        opt = self.options
        self._last_cfg = (build_config(opt, self.paired, opt.index2_file is not None), self.bubbleCircles)
        for e in self._engines():
            e.set_config(self._last_cfg[0])
            set_view_passes(e, (self.cut, self.adapter, self.poly), clear=True)
            if first:
                e.set_circles(self.bubbleCircles)
                e.reset_stats()

    def _sample(self, eng):
        """Pass 1: pre-filter QC on a sample of each file (preprocesser.py:247-251) -> the QC objects of R1 and R2."""
        opt = self.options
        # --adapter_sequence auto: the census of the same reads, with the probes of the mate's column.  Without it nothing of the
        # census is called (probes an engine the caller handed over still has from another run are never looked at)
        if any(self.adapter_auto):
            if not hasattr(eng, "adapter_census"):
                raise RuntimeError("afterqc_amd: --adapter_sequence auto / --adapter_sequence_r2 auto need an engine with adapter_census; "
                                   "%s has none" % type(eng).__name__)
            for mate, which in enumerate((capi.QC_R1_PRE, capi.QC_R2_PRE)):
                eng.set_adapter_probes(which, adapter_detect.probes(mate) if self.adapter_auto[mate] else None)
        r1pre = QualityControl(opt.qc_sample, opt.qc_kmer, eng, capi.QC_R1_PRE, census=self.adapter_auto[0])
        r2pre = QualityControl(opt.qc_sample, opt.qc_kmer, eng, capi.QC_R2_PRE, census=self.adapter_auto[1])
        if not (self.use_text_path and hasattr(eng, "frame")):
            r1pre.statFile(opt.read1_file, fastq.Reader, capi.Batch.from_raw, self.batch_records)
            if self.paired:
                # the R2 file is stat'd through the same single-read path into its own accumulator
                r2pre.statFile(opt.read2_file, fastq.Reader, capi.Batch.from_raw, self.batch_records)
            return r1pre, r2pre
        side, side_err = None, []
        if self.paired and isinstance(eng, capi.Engine) and eng.n_slots >= 2:
            # read 2 is sampled at the same time in slot 1 (a .gz spends most of this pass decoding)
            def _sample_r2():
                try:
                    r2pre.statFileText(opt.read2_file, self.chunk_bytes, slot=1)
                except BaseException as e:       # re-raised on the main thread
                    side_err.append(e)
            side = threading.Thread(target=_sample_r2, name="aqc-sample-r2")
            side.start()
        try:
            r1pre.statFileText(opt.read1_file, self.chunk_bytes)
        finally:
            if side is not None:
                side.join()
        if side_err:
            raise side_err[0]
        if self.paired and side is None:
            r2pre.statFileText(opt.read2_file, self.chunk_bytes)
        return r1pre, r2pre

    def _auto_trim(self, r1pre, r2pre):
        """Every trim option left at -1 is resolved from the pass-1 sample (preprocesser.py:261-280)."""
        opt = self.options
        if opt.trim_front != -1 and opt.trim_tail != -1:
            return
        tf, tt = r1pre.autoTrim()
        if opt.trim_front == -1:
            opt.trim_front = tf
        if opt.trim_tail == -1:
            opt.trim_tail = tt
        if self.paired and opt.trim_pair_same:
            opt.trim_front2 = opt.trim_front
            opt.trim_tail2 = opt.trim_tail
        elif self.paired:
            tf2, tt2 = r2pre.autoTrim()
            if opt.trim_front2 == -1:
                opt.trim_front2 = tf2
            if opt.trim_tail2 == -1:
                opt.trim_tail2 = tt2

    def _detect_adapters(self, eng):
        """--adapter_sequence auto: each asked mate's adapter from the census of its pass-1 sample (adapter_detect) -> self.adapter
        as pass 2 runs it, self.adapter_detect for the statistics.  Nothing found for any mate and none given: no adapter pass."""
        if not any(self.adapter_auto):
            return
        opt = self.options
        n = len(adapter_detect.CANDIDATES)
        self.adapter_detect = {"probe_len": adapter_detect.PROBE_LEN, "min_reads": adapter_detect.MIN_READS,
                               "min_per_mille": adapter_detect.MIN_PER_MILLE}
        found = ["", ""]
        for mate, which in enumerate((capi.QC_R1_PRE, capi.QC_R2_PRE)):
            if not self.adapter_auto[mate]:
                continue
            counts = [int(v) for v in eng.adapter_census_counts(which)]
            rep = adapter_detect.report(mate, counts[1:1 + n], counts[0])
            self.adapter_detect["read%d" % (mate + 1)] = rep
            found[mate] = rep["adapter"]
            held = dict(rep["candidates"]).get(rep["detected"], 0)
            print("%s: read %d adapter %s" % (opt.read2_file if mate else opt.read1_file, mate + 1,
                                              "%s %s (in %d of %d sampled reads)" % (rep["detected"], rep["adapter"], held, rep["sampled"])
                                              if rep["detected"] else "not detected in %d sampled reads: not searched" % rep["sampled"]))
        self.adapter = adapter_config(opt, found)

    def _layout(self):
        """Output layout (preprocesser.py:285-371): makes the folders -> (report folder, gzip the outputs?, per input file
        (read 1, read 2, index 1, index 2) the paths of its good / bad / overlap output; None: not written)."""
        opt = self.options
        good_dir = opt.good_output_folder
        if good_dir is None:
            good_dir = os.path.dirname(opt.read1_file)
        parent = os.path.dirname(os.path.dirname(good_dir + "/"))
        bad_dir = opt.bad_output_folder if opt.bad_output_folder is not None else os.path.join(parent, "bad")
        overlap_dir = opt.overlap_output_folder if opt.overlap_output_folder is not None else os.path.join(parent, "overlap")
        qc_dir = opt.report_output_folder if opt.report_output_folder is not None else os.path.join(parent, "QC")
        for d in (qc_dir, good_dir, bad_dir):
            os.makedirs(d, exist_ok=True)          # (directory mode runs several files at once)
        if opt.store_overlap and (self.paired or not opt.qc_only):
            os.makedirs(overlap_dir, exist_ok=True)   # (single-end + store_overlap: upstream opens the writer without the dir)
        # --store_merged: read 1's third output is the merged file, read 2 and the index files have none
        merged = third_stream_mode(opt, self.paired) == capi.STORE_MERGED and not opt.qc_only
        if merged:
            merged_dir = opt.merged_output_folder if getattr(opt, "merged_output_folder", None) is not None else os.path.join(parent, "merged")
            os.makedirs(merged_dir, exist_ok=True)
        gzip_out = bool(opt.gzip) or opt.read1_file.endswith(".gz")
        ext = ".gz" if gzip_out else ""
        paths = []
        for k, f in enumerate(input_files(opt)):
            if f is None or opt.qc_only:
                paths.append((None, None, None))
                continue
            main = getMainName(f)
            # upstream opens the R1 overlap writer whenever store_overlap is on, the others only when paired
            ovl = opt.store_overlap and (k == 0 or self.paired)
            third = os.path.join(overlap_dir, main + ".overlap.fq" + ext) if ovl else None
            if merged:
                third = os.path.join(merged_dir, main + ".merged.fq" + ext) if k == 0 else None
            paths.append((os.path.join(good_dir, main + ".good.fq" + ext), os.path.join(bad_dir, main + ".bad.fq" + ext), third))
        return qc_dir, gzip_out, paths

    def _pass2(self, eng, paths, gzip_out):
        """Pass 2, the main loop (preprocesser.py:411-631), through the driver the run calls for -> the extra-bases quirk value.
        Text in / text out on the device (aqc_frame / aqc_format); use_text_path=False keeps the host-side framing and writer
        as a cross-check, and an injected engine without the text calls takes that path too."""
        opt = self.options
        indexed = opt.index1_file is not None or opt.index2_file is not None
        self.text_path = self.use_text_path and hasattr(eng, "frame")
        if third_stream_mode(opt, self.paired) == capi.STORE_MERGED and not getattr(eng, "formats_merged", False):
            self.text_path = False      # (an injected engine whose format() knows no merged reads: the host-side writer builds them)
        if self.text_path and self.use_pipe and not indexed and not opt.qc_only and isinstance(eng, capi.Engine):
            extra_bases = self._run_pipe(opt, paths, gzip_out)
            if extra_bases is not None:
                return extra_bases
            # not the regular shape (empty line inside, mates of different lengths, ...): start over, chunk by chunk
            print("afterqc_amd: %s is not of the regular shape the whole-input pipe takes (blank line inside / mates of "
                  "different lengths); running it again through the serial chunk loop" % opt.read1_file, file=sys.stderr)
            self.timing["pipe_fallback"] = True
            for e in self._engines():
                e.reset_stats()
        outs = _Outputs(paths, opt.compression)
        try:
            if not self.text_path:
                return self._run_host(eng, opt, outs)
            return self._run_text_indexed(eng, opt, outs) if indexed else self._run_text(eng, opt, outs)
        finally:
            # (also when the run ends in an exception: what was written up to the record upstream dies at stays written)
            outs.close()

    def _report(self, eng, r1pre, r2pre, extra_bases, qc_dir):
        """Post-filter QC and the counters -> self.stat, QC/<R1 basename>.json and the HTML report next to it."""
        opt = self.options
        t_stats = time.perf_counter()
        # statistics: per-GPU integers summed on the host (only the pipe spreads a run over several engines)
        stat_eng = capi.MergedEngines(self._engines()) if self.extra_engines else eng
        r1post = QualityControl(opt.qc_sample, opt.qc_kmer, stat_eng, capi.QC_R1_POST)
        r2post = QualityControl(opt.qc_sample, opt.qc_kmer, stat_eng, capi.QC_R2_POST)
        r1post.qc()
        if self.paired:
            r2post.qc()
        readLen = r1pre.readLen
        self.stat = self._stats(stat_eng, r1pre, r2pre, r1post, r2post, readLen, extra_bases)
        stat_path = os.path.join(qc_dir, os.path.basename(opt.read1_file) + ".json")
        with open(stat_path, "w") as f:
            f.write(json.dumps(self.stat, sort_keys=True, indent=4, separators=(',', ': ')))
        self.timing["stats_s"] = time.perf_counter() - t_stats
        t_report = time.perf_counter()
        # the HTML report next to it (preprocesser.py:780-783, qcreporter.py).  The FASTQ outputs and the statistics are
        # complete at this point: a problem in the report is reported, it does not fail the run
        try:
            from . import qcreporter
            ovl_hist, _ = stat_eng.histograms(capi.AQC_QC_COLS)
            figures = qcreporter.build_figures(self.stat, opt, r1pre, r2pre, r1post, r2post, ovl_hist, readLen)
            with open(os.path.join(qc_dir, os.path.basename(opt.read1_file) + ".html"), "w") as f:
                f.write(qcreporter.render(self.stat, figures, getattr(opt, "version", "")))
        except Exception as e:      # noqa: BLE001 — whatever it is, the run's results stand
            if os.environ.get("AQC_REPORT_STRICT"):      # the test suites: a broken report must not pass unseen
                raise
            print("afterqc_amd: the HTML report could not be written (%s: %s); outputs and %s are complete"
                  % (type(e).__name__, e, stat_path), file=sys.stderr)
            self.timing["report_error"] = "%s: %s" % (type(e).__name__, e)
        self.timing["report_s"] = time.perf_counter() - t_report

    # ---- pass 2 through the whole-input pipe (aqc_pipe_run) ---------------------------------------------------------------
    def _run_pipe(self, opt, paths, gzip_out):
        """Hands the read file(s) to the C++ pipe: chunks of `chunk_records` records dealt over every engine, outputs written
        in chunk order by its writer thread.  Returns the extra-bases quirk value (preprocesser.py:416-421) or None when the
        pipe met an input it cannot chunk (the caller falls back to the serial chunk loop)."""
        files = [opt.read1_file] + ([opt.read2_file] if self.paired else [])
        engines = self._engines(all_devices=True)
        pipe = capi.Pipe(engines, slots=min([self.pipe_slots] + [e.n_slots for e in engines]), io_threads=self.io_threads)
        try:
            # (fastq.py:23-26: .gz through gzip.open, .bz2 through bz2.BZ2File upstream — here the pipe's own decoders: 1 gzip, 2 bzip2)
            res = pipe.run(files, paths[:len(files)], gzip_in=[1 if f.endswith(".gz") else 2 if f.endswith(".bz2") else 0 for f in files],
                           gzip_out=gzip_out, gzip_level=opt.compression, chunk_records=self.chunk_records, qc_sample=opt.qc_sample,
                           store_overlap=third_stream_mode(opt, self.paired) if self.paired else capi.STORE_OFF)
        except capi.AqcError as e:
            # (an exception inside upstream's loop — capi.RECORD_ERRORS — ends the run at that record: the pipe has written
            #  everything before it and says so; there is nothing to rerun)
            self.used_pipe = e.code in capi.RECORD_ERRORS
            raise
        finally:
            pipe.close()
        self.used_pipe = not res.anomaly
        if res.anomaly:
            return None
        self.timing["pipe_s"] = res.seconds
        self.timing["pipe_threads"] = res.breakdown()
        self.timing["pipe_chunks"] = (int(res.chunks), int(res.fused_chunks))       # (all, placed by the verdict kernel: AQC_FUSED=1)
        # (R1's record that upstream had read and counted before a shorter R2 ended its loop, preprocesser.py:416-421: the pipe
        #  applies fastq.Reader's end-of-file rules itself since round 6)
        return int(res.extra_bases)

    # ---- the body of upstream's loop for one chunk: every serial driver calls this -------------------------------------
    def _judge(self, eng, slot, n, total, wait=True):
        """Verdicts and statistics of the `n` records framed or uploaded into `slot`, `total` records (TOTAL_READS) into the
        run -> (n, stop, death): the records of the chunk that count, whether the loop ends with them, and the AqcError to
        raise once they are written — an exception inside upstream's loop ends its run AT that record (death_record).
        wait=False (the pipelined loop, whose fetch thread meets a death of its own): no host-blocking call but the one
        the sampling kernels need."""
        opt = self.options
        stop, death = False, None
        try:
            limit = capi.UINT64_MAX
            if opt.qc_only:
                # --qc_only stops at the first good record whose 1-based index reaches qc_sample (:630-631):
                # verdicts first (nothing accumulated), then the accumulating run up to that record
                eng.run(slot, 0)
                flags = eng.fetch_results(slot)[:n]["flag"]
                hit = np.flatnonzero((flags == capi.GOOD) & (total + 1 + np.arange(n) >= opt.qc_sample))
                if len(hit):
                    n = int(hit[0]) + 1
                    stop = True
                limit = n
            eng.run(slot, limit)
            # post-filter QC on good records while TOTAL_READS < qc_sample (preprocesser.py:624-627)
            n_qc = n if opt.qc_sample <= 0 else max(0, min(n, opt.qc_sample - 1 - total))
            if n_qc > 0:
                eng.qc_stat(slot, capi.QC_R1_POST, 0, 0, n_qc, 1)
                if self.paired:
                    eng.qc_stat(slot, capi.QC_R2_POST, 1, 0, n_qc, 1)
            # the sampling kernels share per-context scratch: never two chunks at once; and a death surfaces at a host-blocking
            # call: with `wait` here, where it is cut at its record, not in the caller's fetches
            if wait or n_qc > 0 or opt.qc_only:
                eng.sync(slot)
        except capi.AqcError as e:
            k = death_record(eng, slot, e)
            if k is None or k >= n:
                raise
            n, stop, death = k, True, e
        return n, stop, death

    # ---- pass 2, text path with index files (-7 / -5): four lock-stepped inputs, two device slots ---------------------
    def _run_text_indexed(self, eng, opt, outs):
        """Like _run_text, for runs with index files: the reads are framed into slot 0, the index reads into slot 1 (capped
        at the reads' record count), the index records are formatted whole under the reads' verdicts
        (aqc_format_plain).  Rare in practice, so this variant is kept simple: one chunk at a time, fetch and write inline."""
        inputs = [_TextInput(eng, f, self.chunk_bytes) for f in input_files(opt) if f is not None]
        writers = [w for w, f in zip(outs.per_file, input_files(opt)) if f is not None]
        nr = 2 if self.paired else 1                  # inputs[:nr] are the reads, inputs[nr:] the index reads
        hold = [None] * 6
        total = 0
        cur = 0

        def write_streams(slot, group, sizes):
            for q, nbytes in enumerate(sizes):
                if nbytes and q // 3 < len(group) and group[q // 3][q % 3] is not None:
                    group[q // 3][q % 3].write_bytes(fetch_stream(eng, slot, q, nbytes, hold).view[:nbytes])

        try:
            for inp in inputs:
                inp.start_fill(cur, 0)
            while True:
                fills = [inp.wait_fill() for inp in inputs]
                info, reads = frame_inputs(eng, 0, inputs[:nr], fills[:nr], cur, total)
                info_b, index = frame_inputs(eng, 1, inputs[nr:], fills[nr:], cur, total, int(info.n))
                n = int(info_b.n)
                if n < int(info.n):
                    info, reads = frame_inputs(eng, 0, inputs[:nr], fills[:nr], cur, total, n)    # the index chunk holds fewer records
                stop, extra_bases, finished = lock_step(reads + index, info)
                if not stop:
                    advance(inputs, cur, n, reads + index, finished)
                if n:
                    n, cut, death = self._judge(eng, 0, n, total)
                    if not opt.qc_only:
                        mode = third_stream_mode(opt, self.paired)
                        write_streams(0, writers[:nr], eng.format(0, n, mode))
                        write_streams(1, writers[nr:], eng.format_plain(1, 0, n, mode))
                    if death is not None:
                        raise death
                    total += n
                    stop = stop or cut
                if stop:
                    return extra_bases
                cur = 1 - cur
        finally:
            for inp in inputs:
                inp.close()
            for b in hold:
                if b is not None:
                    b.free()

    # ---- pass 2 with host-side framing / formatting (general: barcodes, index files, overlap store, bubbles) ------
    def _run_host(self, eng, opt, outs):
        readers = [fastq.Reader(f) if f is not None else None for f in input_files(opt)]
        total = 0          # TOTAL_READS so far
        extra_bases = 0    # R1 bases read for a record that a shorter mate file then cut off (:416-421)
        stop = False
        slot = 0
        try:
            while not stop:
                rbs = [r.next_batch(self.batch_records) if r is not None else None for r in readers]
                if rbs[0] is None:
                    break
                # lock step over whole batches (the rule is stated by lock_step): the first file to run dry ends the loop, and
                # R1's record was already counted into TOTAL_BASES by then
                n = min(rbs[k].n if rbs[k] is not None else 0 for k in range(4) if readers[k] is not None)
                if n < rbs[0].n:
                    extra_bases = int(rbs[0].seq_len[n])
                    stop = True
                if n == 0:
                    break
                batch = capi.Batch.from_raw(rbs[0], rbs[1] if self.paired else None, first_index=total)
                if n < batch.n:
                    batch.n = n
                if opt.debubble:
                    self._aux(batch, rbs[0])
                eng.upload(slot, batch)
                n, cut, death = self._judge(eng, slot, n, total)
                stop = stop or cut
                if not opt.qc_only:
                    qviews = None
                    if batch.qlen1 is not None:
                        qviews = [eng.fetch_quality_views(slot, 0), eng.fetch_quality_views(slot, 1) if self.paired else None]
                    self._write(outs, rbs, eng.fetch_results(slot)[:n], n, qviews)
                if death is not None:
                    raise death
                total += n
        finally:
            for r in readers:
                if r is not None:
                    r.close()
        return extra_bases

    # ---- pass 2, text in / text out: framing and formatting on the device -------------------
    def _run_text(self, eng, opt, outs):
        """The loop of preprocesser.py:411-631 over raw text chunks.  Per chunk the host only moves bytes: file ->
        page-locked buffer -> aqc_frame (records found on the device) -> aqc_run / aqc_qc_stat -> aqc_format
        (good / bad text built on the device) -> page-locked buffer -> file.  File reads and writes run on side
        threads while the main thread sits in the (GIL-free) C-ABI calls."""
        files = [opt.read1_file] + ([opt.read2_file] if self.paired else [])
        inputs = [_TextInput(eng, f, self.chunk_bytes) for f in files]
        n_slots = min(2, getattr(eng, "n_slots", 1))
        mode = third_stream_mode(opt, self.paired)
        sink = _TextSink(eng, outs.per_file[:len(files)], n_slots, mode)
        total = 0
        slot = 0
        cur = 0
        try:
            for inp in inputs:
                inp.start_fill(cur, 0)
            while True:
                fills = [inp.wait_fill() for inp in inputs]          # (bytes in buffer `cur`, final)
                sink.acquire_slot(slot)                               # its previous chunk has left the device
                info, state = frame_inputs(eng, slot, inputs, fills, cur, total)
                n = int(info.n)
                stop, extra_bases, finished = lock_step(state, info)
                if not stop:
                    advance(inputs, cur, n, state, finished)
                if n:
                    n, cut, death = self._judge(eng, slot, n, total, wait=False)
                    stop = stop or cut
                    if opt.qc_only:
                        sink.release_slot(slot)
                        if death is not None:
                            raise death
                    else:
                        sink.emit(slot, eng.format(slot, n, mode), death)   # (the fetch thread releases the slot)
                    total += n
                else:
                    sink.release_slot(slot)
                if stop:
                    return extra_bases
                cur = 1 - cur
                slot = (slot + 1) % n_slots
        finally:
            sink.close()
            for inp in inputs:
                inp.close()

    # ---- output formatting (writeReads, preprocesser.py:206-232; fastq.Writer.writeLines) ------------
    def _write(self, outs, rbs, results, n, qviews=None):
        """qviews: per mate (starts, lengths) of the quality-string slices (Engine.fetch_quality_views) when some record's quality
        line is not as long as its sequence line; None: the slices of the reads"""
        opt = self.options
        paired = self.paired
        vlen = len(opt.barcode_verify)
        bl = opt.barcode_length
        store = opt.store_overlap
        merge = third_stream_mode(opt, paired) == capi.STORE_MERGED
        chunks = [[[], [], []] for _ in range(4)]      # per file: good, bad, overlap byte pieces
        rb1, rb2, rbi1, rbi2 = rbs
        flags = results["flag"]
        for i in range(n):
            r = results[i]
            flag = int(flags[i])
            name1, s1, p1, q1 = rb1.record(i)
            if paired:
                name2, s2, p2, q2 = rb2.record(i)
            bc = int(r["barcode"])
            moved = opt.barcode and flag not in (capi.BADBCD1, capi.BADBCD2)
            if moved:
                # moveBarcodeToName (barcodeprocesser.py:34-45): '@' + barcode + name[first ':' :]
                # single-end moves the DESIGN length (preprocesser.py:444), paired the detected lengths (:452)
                b1 = (bc & 15) - 2 + bl if paired else bl
                name1 = b"@" + s1[0:b1] + name1[name1.find(b":"):]
                if paired:
                    b2 = (bc >> 4) - 2 + bl
                    name2 = b"@" + s2[0:b2] + name2[name2.find(b":"):]
            st, ln = int(r["start1"]), int(r["len1"])
            qs, ql = (st, ln) if qviews is None else (int(qviews[0][0][i]), int(qviews[0][1][i]))
            s1 = bytearray(s1[st:st + ln]); q1 = bytearray(q1[qs:qs + ql])
            if paired:
                st2, ln2 = int(r["start2"]), int(r["len2"])
                qs2, ql2 = (st2, ln2) if qviews is None else (int(qviews[1][0][i]), int(qviews[1][1][i]))
                s2 = bytearray(s2[st2:st2 + ln2]); q2 = bytearray(q2[qs2:qs2 + ql2])
            ov = int(r["overlap_len"])
            ne = int(r["n_edits"])
            corrected = 0
            # (each string is edited at its OWN index, preprocesser.py:575-592: the quality strings from their own ends — the
            #  same positions as the bases' unless a quality line has a length of its own; a negative index wraps, as upstream)
            for k in range(ne):
                e = r["edits"][k]
                o = int(e["o"]); kind = int(e["kind"])
                if kind == capi.EDIT_FIX_R2:
                    s2[ln2 - 1 - o] = int(e["base"]); q2[len(q2) - 1 - o] = int(e["qual"]); corrected += 1
                elif kind == capi.EDIT_FIX_R1:
                    s1[ln - ov + o] = int(e["base"]); q1[len(q1) - ov + o] = int(e["qual"]); corrected += 1
                else:
                    q2[len(q2) - 1 - o] = 33; q1[len(q1) - ov + o] = 33
            which = 0 if flag == capi.GOOD else 1
            if which == 1:
                fb = FLAG_BYTES[flag]
                name1 = b"@" + fb + name1[1:]
                if paired:
                    name2 = b"@" + fb + name2[1:]
            if (store or merge) and paired and not opt.no_overlap and flag == capi.GOOD and ov > 30:
                dist = int(r["distance"])
                if merge:
                    # --store_merged: the same pairs, written once (stream 2 of read 1)
                    rec = merged_record(name1, s1, p1, q1, s2, q2, ov) if dist == 0 or dist == corrected else None
                    if rec is not None:
                        chunks[0][2].append(rec)
                elif dist == 0 or dist == corrected:
                    # getOverlap (preprocesser.py:78-84): the last overlap_len bases of both reads
                    chunks[0][2].append(name1 + b"\n" + bytes(s1[ln - ov:]) + b"\n" + p1 + b"\n" + bytes(q1[len(q1) - ov:]) + b"\n")
                    chunks[1][2].append(name2 + b"\n" + bytes(s2[ln2 - ov:]) + b"\n" + p2 + b"\n" + bytes(q2[len(q2) - ov:]) + b"\n")
                    for k, rbx in ((2, rbi1), (3, rbi2)):
                        if rbx is not None:
                            chunks[k][2].append(b"\n".join(rbx.record(i)) + b"\n")
            chunks[0][which].append(name1 + b"\n" + bytes(s1) + b"\n" + p1 + b"\n" + bytes(q1) + b"\n")
            if paired:
                chunks[1][which].append(name2 + b"\n" + bytes(s2) + b"\n" + p2 + b"\n" + bytes(q2) + b"\n")
            for k, rbx in ((2, rbi1), (3, rbi2)):
                if rbx is not None:
                    rec = rbx.record(i)
                    if which == 1:
                        rec[0] = b"@" + FLAG_BYTES[flag] + rec[0][1:]
                    chunks[k][which].append(b"\n".join(rec) + b"\n")
        for k in range(4):
            for which, group in ((0, outs.good), (1, outs.bad), (2, outs.overlap)):
                if group[k] is not None and chunks[k][which]:
                    group[k].write_bytes(b"".join(chunks[k][which]))

    # ---- statistics -> JSON (preprocesser.py:660-778) ---------------------------------------------------
    def _stats(self, eng, r1pre, r2pre, r1post, r2post, readLen, extra_bases):
        opt = self.options
        C = eng.counters()
        c = lambda k: int(C[k])
        f = lambda k: int(C[capi.C_FLAG0 + k])
        total_reads = c(capi.C_TOTAL_READS)
        good_reads = c(capi.C_GOOD_READS)
        summary = {
            'total_bases': c(capi.C_TOTAL_BASES) + extra_bases,
            'good_bases': c(capi.C_GOOD_BASES),
            'total_reads': total_reads,
            'good_reads': good_reads,
            'bad_reads': total_reads - good_reads,
            'bad_reads_with_bad_barcode': f(capi.BADBCD1) + f(capi.BADBCD2),
            'bad_reads_with_reads_in_bubble': f(capi.BADBBL),
            'bad_reads_with_bad_read_length': f(capi.BADLEN) + f(capi.BADTRIM1) + f(capi.BADTRIM2),
            'bad_reads_with_polyX': f(capi.BADPOL),
            'bad_reads_with_low_quality': f(capi.BADLQC),
            'bad_reads_with_too_many_N': f(capi.BADNCT),
            'bad_reads_with_bad_overlap': f(capi.BADMISMATCH) + f(capi.BADDIFF),   # BADINDEL is always 0 upstream
            'readlen': readLen,
        }
        stat = {"afterqc_main_summary": summary, "command": makeDict(opt)}
        pairs = [("read1_prefilter", r1pre), ("read1_postfilter", r1post)]
        if self.paired:
            pairs += [("read2_prefilter", r2pre), ("read2_postfilter", r2post)]
        stat["kmer_content"] = {k: q.json_top_kmers(10) for k, q in pairs}
        stat["base_quality"] = {k: q.json_base_quality() for k, q in pairs}
        stat["mean_quality"] = {k: q.json_mean_quality() for k, q in pairs}
        stat["base_content"] = {k: q.json_base_content() for k, q in pairs}
        stat["gc_content"] = {k: q.json_gc_content() for k, q in pairs}
        if self.paired:
            overlapped = c(capi.C_OVERLAPPED)
            base_sum = c(capi.C_OVERLAP_BASE_SUM)
            _, dist_hist = eng.histograms(capi.AQC_QC_COLS)
            ov = {
                'overlapped_pairs': overlapped,
                # python-2 integer division upstream: float(OVERLAP_LEN_SUM/OVERLAPPED) (preprocesser.py:752)
                'average_overlap_length': float(c(capi.C_OVERLAP_LEN_SUM) // overlapped) if overlapped > 0 else 0.0,
                'bad_mismatch_reads': f(capi.BADMISMATCH),
                'bad_diff': f(capi.BADDIFF),
                'bad_indel_reads': 0,
                'corrected_reads': c(capi.C_READ_CORRECTED),
                'corrected_bases': c(capi.C_BASE_CORRECTED),
                'skipped_correction_bases': c(capi.C_BASE_SKIPPED_CORRECTION),
                'zero_qual_masked': c(capi.C_BASE_ZERO_QUAL_MASKED),
                'zero_qual_skipped': c(capi.C_BASE_ZERO_QUAL_MASKED),
                'trimmed_adapter_bases': c(capi.C_TRIMMED_ADAPTER_BASE),
                'trimmed_adapter_reads': c(capi.C_TRIMMED_ADAPTER_READ),
                'error_rate': float(c(capi.C_OVERLAP_BASE_ERR)) / float(base_sum) if base_sum > 0 else 0.0,
                'edit_distance_histogram': [int(v) for v in dist_hist[0:min(10, readLen + 1)]],
            }
            mtx = {}
            for i, a in enumerate(ALL_BASES):
                mtx[a] = {b: c(capi.C_ERR_MATRIX0 + 4 * i + j) for j, b in enumerate(ALL_BASES) if b != a}
            ov['error_matrix'] = mtx
            stat["afterqc_overlap"] = ov
        if self.cut is not None:
            n = [int(v) for v in eng.cut_stats()]
            stat["quality_cut"] = {
                'cut_front': bool(self.cut.front), 'cut_tail': bool(self.cut.tail), 'cut_right': bool(self.cut.right),
                'cut_window_size': int(self.cut.window), 'cut_mean_quality': int(self.cut.mean_quality),
                'read1_cut_reads': n[0], 'read1_cut_bases': n[1], 'read2_cut_reads': n[2], 'read2_cut_bases': n[3],
            }
        if self.adapter is not None:
            n = [int(v) for v in eng.adapter_stats()]
            a1, a2 = self.adapter.adapters()
            stat["adapter_trim"] = {
                'adapter_sequence': a1.decode(), 'adapter_sequence_r2': a2.decode(), 'adapter_min_overlap': int(self.adapter.min_overlap),
                'read1_trimmed_reads': n[0], 'read1_trimmed_bases': n[1], 'read2_trimmed_reads': n[2], 'read2_trimmed_bases': n[3],
            }
        if self.adapter_detect is not None:
            stat["adapter_detect"] = self.adapter_detect
        if self.poly is not None:
            n = [int(v) for v in eng.poly_stats()]
            stat["poly_trim"] = {
                'trim_poly_g': bool(getattr(opt, "trim_poly_g", False)), 'poly_g_min_len': int(getattr(opt, "poly_g_min_len", 10)),
                'trim_poly_x': bool(getattr(opt, "trim_poly_x", False)), 'poly_x_min_len': int(getattr(opt, "poly_x_min_len", 10)),
                'read1_trimmed_reads': n[0], 'read1_trimmed_bases': n[1], 'read2_trimmed_reads': n[2], 'read2_trimmed_bases': n[3],
            }
        return stat
