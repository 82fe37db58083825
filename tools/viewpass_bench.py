"""What tools/qcut_bench.py, tools/adapter_bench.py and tools/poly_bench.py share: the verdict configuration, the loads and the
batch of one, generated reads kept as .npy, the two-context alternating loop around aqc_run with the view pass's own time beside
the verdict kernel's, the passes' own times alone, the device step on text resident in HBM, the single run for a profiler, and the
rate of a pass as a share of the HBM peak.  Each tool keeps its input, its option and its output lines.  (afterqc_amd is imported
inside the functions: a tool may first put another checkout in front of this one.)"""
import os
import time

PEAK = 8.0e12          # HBM_PEAK_GBS of bench.py
A1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
A2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
LOADS = {"se150": (150, False), "pe150": (150, True), "pe300": (300, True)}
KEYS = ("seq1", "qual1", "len1", "seq2", "qual2", "len2")


def cached_input(cache, name, generate):
    """generate() -> the six arrays of synth.make_pairs; with a cache directory they are kept there as <name>_<key>.npy, so that
    the processes of a job make them once"""
    import numpy as np
    stem = os.path.join(cache, name) if cache else ""
    if stem and all(os.path.exists("%s_%s.npy" % (stem, k)) for k in KEYS):
        return {k: np.load("%s_%s.npy" % (stem, k)) for k in KEYS}
    d = generate()
    if stem:
        os.makedirs(cache, exist_ok=True)
        for k in KEYS:
            np.save("%s_%s.npy" % (stem, k), d[k])
    return d


def batch_of(d, paired):
    from afterqc_amd import capi
    if paired:
        return capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"], d["seq2"], d["qual2"], d["len2"])
    return capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"])


def moved_bytes(L, paired, n):
    """what a sequence-line pass must move: per mate the sequence bytes, a length word, an offset word and 4 bytes of view"""
    return (2 if paired else 1) * (L + 12) * n


def base_config(paired=True, trim=(0, 0)):
    from afterqc_amd import capi
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.seq_len_req, cfg.poly_size_limit, cfg.allow_mismatch_in_poly = 35, 35, 2
    cfg.qualified_quality_phred, cfg.unqualified_base_limit, cfg.n_base_limit = 15, 60, 5
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    cfg.trim_front = cfg.trim_front2 = trim[0]
    cfg.trim_tail = cfg.trim_tail2 = trim[1]
    return cfg


def prepare(eng, batch, paired, set_pass, trim=(0, 0)):
    """the verdict configuration, the passes as set_pass(engine) leaves them, the counts at zero and the batch in slot 0"""
    eng.set_config(base_config(paired, trim))
    set_pass(eng)
    eng.reset_stats()
    eng.upload(0, batch)


def of_peak(moved, ms):
    return moved / (ms * 1e-3) / PEAK


def alternate(engines, a, pass_tag, pass_ms):
    """a.warmup + a.reps aqc_run on slot 0 of each of `engines` ((tag, engine), ...) in turn -> the verdict kernel's times per tag
    (HIP events around AQC_K_FILTER_OVERLAP) and pass_ms(engine) of the context `pass_tag`, warm-up left out"""
    from afterqc_amd import capi
    ms, pms = {}, []
    for k in range(a.warmup + a.reps):
        for tag, eng in engines:
            eng.timing_reset(0)
            eng.run(0)
            t, cnt = eng.timing_mean(0)
            assert cnt[capi.K_FILTER_OVERLAP] == 1
            if k >= a.warmup:
                ms.setdefault(tag, []).append(float(t[capi.K_FILTER_OVERLAP]))
                if tag == pass_tag:
                    pms.append(pass_ms(eng))
    return ms, pms


def verdict_rows(engines, ms, pms, pass_tag, load, n, moved, tag_width, pass_width):
    """one line per context: the verdict kernel's median / min / spread and deferred share; behind it, for the context with the
    pass on, the pass's median / min and its share of the peak over `moved` bytes"""
    import numpy as np
    for tag, eng in engines:
        v = np.array(ms[tag])
        row = "  %-6s %-*s %5d %10.4f %9.4f %7.3f %9.5f" % (load, tag_width, tag, eng.last_verdict_words(0), float(np.median(v)), float(v.min()),
                                                           float(v.max() / v.min()), eng.last_deferred(0) / n)
        if tag == pass_tag:
            c = np.array(pms)
            row += " | %*.4f %9.4f %8.4f" % (pass_width, float(np.median(c)), float(c.min()), of_peak(moved, float(np.median(c))))
        print(row, flush=True)


def pass_times(contexts, a):
    """a.warmup + a.reps aqc_run on slot 0 of each of `contexts` ((engine, pass_ms), ...) in turn -> per context the times
    pass_ms(engine) gave, warm-up left out"""
    import numpy as np
    t = [[] for _ in contexts]
    for k in range(a.warmup + a.reps):
        for i, (eng, pass_ms) in enumerate(contexts):
            eng.run(0)
            if k >= a.warmup:
                t[i].append(pass_ms(eng))
    return [np.array(v) for v in t]


def once(a, d, paired, set_pass, ms_name):
    """a.reps aqc_run on the reads `d` with the pass set_pass(engine) switches on, for a profiler's kernel trace"""
    from afterqc_amd import capi
    eng = capi.Engine(0, 1)
    prepare(eng, batch_of(d, paired), paired, set_pass)
    for _ in range(a.reps):
        eng.run(0)
    print("%s: %d aqc_run, %s of the last %.4f" % (a.load, a.reps, ms_name, getattr(eng, ms_name)(0)), flush=True)
    eng.close()


def step(a, make_input, label, set_pass, ms_name):
    """the device step on 2 x 150 and 2 x 300 of make_input(L) with the passes as set_pass(engine) leaves them: a step_line each,
    the pass's own time of the last run behind it"""
    from afterqc_amd import capi
    eng = capi.Engine(0, 2)
    for L in (150, 300):
        d = make_input(L)
        eng.set_config(base_config())
        set_pass(eng)
        eng.reset_stats()
        v, sizes, _ = device_step(eng, d, L, a)
        print("%s  %s %.4f" % (step_line(label, L, v, sizes), ms_name, getattr(eng, ms_name)(0)), flush=True)
    eng.close()


def device_step(eng, d, L, a):
    """the pairs of `d` as text resident in HBM, then a.warmup + a.reps of aqc_reframe -> aqc_run -> aqc_format with the slot
    synced -> (wall ms per timed step, the sizes of the last format, records)"""
    import numpy as np
    from afterqc_amd import synth
    n_rec = len(d["len1"])
    w = synth.fixed_record_width(L)
    texts = []
    for mate in (1, 2):
        hb = eng.host_buffer(n_rec * w + 4096)
        _, nbytes = synth.render_fastq_fixed(d["seq%d" % mate], d["qual%d" % mate], mate, out=hb.array)
        texts.append((hb, nbytes))
    info = eng.frame(0, texts[0][0].array, texts[0][1], True, texts[1][0].array, texts[1][1], True)
    assert int(info.n) == n_rec
    t = []
    for k in range(a.warmup + a.reps):
        eng.sync(0)
        t0 = time.perf_counter()
        eng.reframe(0)
        eng.run(0)
        sizes = eng.format(0, n_rec, False)
        eng.sync(0)
        if k >= a.warmup:
            t.append(1000.0 * (time.perf_counter() - t0))
    return np.array(t), sizes, n_rec


def step_line(label, L, v, sizes):
    import numpy as np
    return "%-16s pe%-4d device_step ms min %.4f median %.4f max %.4f  good bytes %d" % (label, L, float(v.min()), float(np.median(v)), float(v.max()),
                                                                                       int(sizes[0] + sizes[3]))
