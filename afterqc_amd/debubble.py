#!/usr/bin/env python3
"""The debubble pre-pass of `after.py -d DIR --debubble` (after.py:177-184, 207-212): debubble.debubbleDir ->
BubbleProcesser -> BubbleDetector -> CircleDetector, with the reference's outputs and quirks.

  python -m afterqc_amd.debubble -i DIR -o OUT -p 20 -d on

Per FASTQ file of the folder (fastq.isFastq: R1, R2, I1, I2 and Undetermined* alike) every read goes through countPoly
(bubbleprocesser.py:385-397); for the polyX reads the Illumina name gives [lane, surface, swath, camera, tile, x, y,
ord(base), count, tile_no] (:348-383).  On the device that census is aqc_frame -> aqc_poly_census (HIP, aqc_census.hpp); the
files are dealt over the visible GPUs, one context per worker, like processDir.  `census_host` is the same census in numpy
for machines without a GPU.  Then, on the host and in upstream's order: calcMaxMin, three stable sorts (surface,
tile_no % 10000, lane), poly_X.csv, the per-tile CSVs grouped by tile_no % 10000 (the file name takes the lane of the group
before it: upstream's laneOfLastTile), per tile BubbleDetector's density filter and region growing, and the flowcell maps
of drawImages.  CircleDetector.__init__ empties its own records (circledetector.py:19), so the first cluster of >= 150 points
raises ZeroDivisionError upstream; here too, after the CSV of that tile, and before any image or circles.csv is written.

Deviations: a polyX read whose name makes upstream's int() raise kills its child process upstream and the
parent then waits forever in queue.get(); here the pass raises ValueError before anything is written.  A read longer than
AQC_MAX_READ_LEN fails the pass (AqcError / ValueError) instead of being counted.  BAM / CRAM (statFileBam) are unreachable
from after.py (isFastq filters them out) and are left out.
"""
import os
import queue
import re
import threading
import time
from optparse import OptionParser

import numpy as np

from . import fastq

MAX_READ_LEN = 1000                                  # AQC_MAX_READ_LEN
NAME_RE = re.compile(rb'\S+\:\d+\:\S+\:\d+\:\d+\:\d+\:\d+')     # bubbleprocesser.py:358, on the name bytes (python 2 str)
INT_RE = re.compile(rb'[+-]?[0-9]+\Z')               # what int() takes of a field the pattern can produce
STATUS_OK, STATUS_NO_NAME, STATUS_RAISE = 0, 1, 2      # AQC_CENSUS_*
HEADER = "lane,surface,swath,camera,tile,xpos,ypos,base,count, tile_no\n"
SKIP_MESSAGE = 'Error happened with debubble function, just skip it now since it will not affect other features'


class CensusNameError(ValueError):
    """a polyX read whose name upstream's int() / tile_no[k] raises on (upstream: the file's child dies, the pass hangs)"""


def parse_name(name):
    """statFileFastq's name handling (bubbleprocesser.py:361-381) -> (status, [lane, surface, swath, camera, tile, x, y],
    tile_no)"""
    m = NAME_RE.search(name)
    if not m:
        return STATUS_NO_NAME, None, None
    items = m.group().split(b":")
    tile_no = items[4]
    if len(tile_no) < 4 or not tile_no.isdigit():
        return STATUS_RAISE, None, None
    if not all(INT_RE.match(items[k]) for k in (3, 5, 6)):
        return STATUS_RAISE, None, None
    return STATUS_OK, [int(items[3]), int(tile_no[0:1]), int(tile_no[1:2]), int(tile_no[2:3]), int(tile_no[3:]),
                       int(items[5]), int(items[6])], int(tile_no)


def _records_from(index, status, base, count, names):
    """the hits of one file in record order -> upstream's records; a name that raises ends the pass"""
    recs = []
    for k in np.argsort(index, kind="stable"):
        st = int(status[k])
        if st == STATUS_NO_NAME:
            continue
        if st == STATUS_RAISE:
            raise CensusNameError("read %d: a polyX read whose name int() rejects (upstream: ValueError in the census child, "
                             "which then never reports)" % int(index[k]))
        fields, tile_no = names(k)
        recs.append(fields + [int(base[k]), int(count[k]), tile_no])
    return recs


# ---------------------------------------------------------------------------------------------------------------------
# the census on the host (numpy): the CPU engine, and the check the device path is measured against
# ---------------------------------------------------------------------------------------------------------------------
_ATCG = np.zeros(256, dtype=np.int8) - 1
for _i, _c in enumerate(b"ATCG"):
    _ATCG[_c] = _i


def census_host(text, seq_off, seq_len, name_off, name_len, poly_max, first_index=0):
    """countPoly + the name fields for framed records inside `text` (uint8).  Returns a dict of arrays in record order
    (index, status, base, count) and a `names(k)` callable for hit k.  Every maximal run of equal bytes of the text is
    found at once; runs of A / T / C / G of at least poly_max that start inside a sequence line are that read's
    candidates (a run cannot leave its line: '\\n' or a stripped blank ends it); per read the first run of the first
    base in A, T, C, G order wins."""
    if poly_max < 1:
        raise ValueError("poly_max must be >= 1")
    seq_off = np.asarray(seq_off, dtype=np.int64)
    seq_len = np.asarray(seq_len, dtype=np.int64)
    n = len(seq_off)
    if n and int(seq_len.max()) > MAX_READ_LEN:
        raise ValueError("a read is longer than AQC_MAX_READ_LEN (%d)" % MAX_READ_LEN)
    empty = dict(index=np.zeros(0, np.uint64), status=np.zeros(0, np.uint8), base=np.zeros(0, np.uint8),
                 count=np.zeros(0, np.int64), names=None)
    if n == 0:
        return empty
    end = int(seq_off[-1] + seq_len[-1])
    t = np.asarray(text[:end + 1], dtype=np.uint8)
    cut = np.flatnonzero(t[1:] != t[:-1]) + 1
    starts = np.concatenate(([0], cut))
    lens = np.diff(np.concatenate((starts, [len(t)])))
    b = _ATCG[t[starts]]
    keep = (lens >= poly_max) & (b >= 0)
    starts, lens, b = starts[keep], lens[keep], b[keep]
    rec = np.searchsorted(seq_off, starts, side="right") - 1
    ok = rec >= 0
    ok[ok] &= starts[ok] < seq_off[rec[ok]] + seq_len[rec[ok]]
    starts, lens, b, rec = starts[ok], lens[ok], b[ok], rec[ok]
    if len(rec) == 0:
        return empty
    order = np.lexsort((starts, b, rec))
    first = order[np.concatenate(([True], rec[order][1:] != rec[order][:-1]))]
    hit = rec[first]
    status = np.zeros(len(hit), dtype=np.uint8)
    parsed = []
    for j, r in enumerate(hit):
        o = int(name_off[r])
        st, fields, tile_no = parse_name(bytes(text[o:o + int(name_len[r])]))
        status[j] = st
        parsed.append((fields, tile_no))
    return dict(index=(hit + first_index).astype(np.uint64), status=status, base=np.frombuffer(b"ATCG", np.uint8)[b[first]],
                count=lens[first].astype(np.int64), names=lambda k: parsed[k])


def stat_file_host(path, poly_max, batch=1 << 18):
    """statFileFastq (bubbleprocesser.py:348-383) with census_host"""
    rd = fastq.Reader(path)
    recs = []
    total = 0
    try:
        while True:
            rb = rd.next_batch(batch)
            if rb is None:
                break
            c = census_host(rb.text, rb.seq_off, rb.seq_len, rb.name_off, rb.name_len, poly_max, total)
            recs += _records_from(c["index"], c["status"], c["base"], c["count"], c["names"])
            total += rb.n
    finally:
        rd.close()
    return recs


# ---------------------------------------------------------------------------------------------------------------------
# the census on the device: aqc_frame -> aqc_poly_census per chunk of the file
# ---------------------------------------------------------------------------------------------------------------------
def stat_file_device(eng, path, poly_max, chunk_bytes=64 << 20, slot=0):
    """statFileFastq on one GPU context: the file's text in chunks (fastq.open_binary: the pipe's readers for plain and .gz,
    BZ2File for .bz2) -> aqc_frame (single-end) -> aqc_poly_census -> hits, in record order"""
    from .preprocesser import _TextInput
    inp = _TextInput(eng, path, chunk_bytes)
    recs = []
    total = 0
    cur = 0
    try:
        inp.start_fill(cur, 0)
        while True:
            nbytes, final = inp.wait_fill()
            buf = inp.bufs[cur].array
            info = eng.frame(slot, buf, nbytes, final, first_index=total)
            n = int(info.n)
            stop = bool(info.eof1 or final) and int(info.avail1) == n
            hits = eng.fetch_census(slot, eng.poly_census(slot, poly_max)) if n else None
            if hits is not None and len(hits):
                def names(k, h=hits, b=buf):
                    if h["wide"][k]:                      # a field beyond 18 digits: int() of the name bytes
                        o = int(h["name_off"][k])
                        _, fields, tile_no = parse_name(bytes(b[o:o + int(h["name_len"][k])]))
                        return fields, tile_no
                    return ([int(h["lane"][k]), int(h["surface"][k]), int(h["swath"][k]), int(h["camera"][k]), int(h["tile"][k]),
                             int(h["x"][k]), int(h["y"][k])], int(h["tile_no"][k]))
                recs += _records_from(hits["index"], hits["status"], hits["base"], hits["count"], names)
            total += n
            if stop:
                break
            if n == 0 and not final and not info.eof1 and int(info.avail1) == 0:
                inp.grow(cur)                               # not even one record fits the buffer
            inp.carry(cur, int(info.consumed1), nbytes, final, bool(info.eof1))
            cur = 1 - cur
    finally:
        inp.close()
    return recs


def census_files(files, poly_max, engine=None):
    """the polyX records of every file, joined in listing order.  engine: None = HIP, the files dealt over
    after.visible_devices() (one context per worker); "host" = census_host; or a factory(device) -> Engine"""
    if engine == "host":
        return [stat_file_host(f, poly_max) for f in files]
    from . import capi
    from .after import visible_devices
    devs = [0] if callable(engine) else visible_devices()
    todo = queue.Queue()
    for k, f in enumerate(files):
        todo.put((k, f))
    out = [None] * len(files)
    errors = []

    def worker(device):
        eng = None
        try:
            while True:
                try:
                    k, f = todo.get_nowait()
                except queue.Empty:
                    return
                if eng is None:
                    eng = engine(device) if callable(engine) else capi.Engine(device, 1)
                print("start: " + f + "\n")
                out[k] = stat_file_device(eng, f, poly_max)
                print("finished " + f + " with " + str(len(out[k])) + " polyX records")
        except BaseException as e:              # reported once every worker has stopped
            errors.append((k, e))
        finally:
            if eng is not None and not callable(engine):
                eng.close()

    threads = [threading.Thread(target=worker, args=(devs[d % len(devs)],)) for d in range(max(1, min(len(devs), len(files))))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise min(errors, key=lambda e: e[0])[1]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# BubbleDetector.detect (bubbledetector.py:30-62) up to the CircleDetector call
# ---------------------------------------------------------------------------------------------------------------------
SCOPE, MIN_POLY, MIN_POINTS = 500.0, 30, 150


def _pairs(x, y):
    """all (i, j), i and j included, with (xi - xj)^2 + (yi - yj)^2 < 500^2: 500-unit buckets, the 3 x 3 around each point"""
    cx, cy = x // 500, y // 500
    key = cx * (1 << 32) + cy
    order = np.argsort(key, kind="stable")
    skey = key[order]
    uk, ustart = np.unique(skey, return_index=True)
    uend = np.append(ustart[1:], len(skey))
    I, J = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            nk = (cx + dx) * (1 << 32) + (cy + dy)
            pos = np.searchsorted(uk, nk)
            pos_c = np.minimum(pos, len(uk) - 1)
            found = (pos < len(uk)) & (uk[pos_c] == nk)
            s = np.where(found, ustart[pos_c], 0)
            m = np.where(found, uend[pos_c] - ustart[pos_c], 0)
            tot = int(m.sum())
            if tot == 0:
                continue
            ii = np.repeat(np.arange(len(x)), m)
            first = np.repeat(np.cumsum(m) - m, m)
            jj = order[np.repeat(s, m) + (np.arange(tot) - first)]
            d2 = (x[ii] - x[jj]) ** 2 + (y[ii] - y[jj]) ** 2
            near = d2 < 250000
            I.append(ii[near])
            J.append(jj[near])
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(I), np.concatenate(J)


def detect_tile(records, xmax, ymax):
    """BubbleDetector.detect for one tile group: polyG records with count >= 30, neighbour sums within radius 500, the
    records below 4 x the mean dropped, region growing; True when a cluster of >= 150 points survives (upstream then hands
    it to CircleDetector, whose detectDirectly divides by its emptied record list)"""
    g = [r for r in records if r[7] == ord('G') and r[8] >= MIN_POLY]
    if any(int(r[5] / 300.0) < 0 or int(r[6] / 300.0) < 0 for r in g):
        raise KeyError("a polyG record left of / above the tile's grid (bubbledetector.py:189-192)")
    total = sum(r[8] for r in g)
    percent = (SCOPE * SCOPE * 3.1415926) / float(xmax * ymax)          # calcMeanCount (ZeroDivisionError as upstream)
    min_neighbour = percent * total * 4
    if len(g) < MIN_POINTS:
        return False
    x = np.array([r[5] for r in g], dtype=np.int64)
    y = np.array([r[6] for r in g], dtype=np.int64)
    cnt = np.array([r[8] for r in g], dtype=np.float64)
    I, J = _pairs(x, y)
    dens = np.bincount(I, weights=cnt[J], minlength=len(g))
    keep = np.flatnonzero(dens >= min_neighbour)                       # filterRecord(4): drops neighbour < min
    if len(keep) < MIN_POINTS:
        return False
    I, J = _pairs(x[keep], y[keep])
    lab = np.arange(len(keep))
    while True:                                                        # connected components: min-label propagation
        new = lab.copy()
        np.minimum.at(new, I, lab[J])
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return int(np.bincount(lab).max()) >= MIN_POINTS


# ---------------------------------------------------------------------------------------------------------------------
# BubbleProcesser.run (bubbleprocesser.py:28-74) after the census
# ---------------------------------------------------------------------------------------------------------------------
def write_records(filename, records):
    with open(filename, "w") as f:
        f.write(HEADER)
        f.write("".join(",".join(str(x) for x in r) + "\n" for r in records))


COLORS = {ord('A'): (255, 0, 0), ord('T'): (0, 255, 0), ord('C'): (0, 0, 255), ord('G'): (150, 60, 240)}


def draw_lane(records, max_value, output, Image):
    """BubbleProcesser.draw (bubbleprocesser.py:170-281) for one lane: per camera an image, each polyX read blended
    into the pixel of its place on the flowcell in record order (the int() / min(255, ...) arithmetic of :243-245; values
    below 0 stay in the buffer and PIL clips them when the image is built).  Returns False where upstream's child dies
    (an offset outside the image: IndexError) — that lane then gets no image."""
    lane = records[0][0]
    swath_max, camera_max, tile_max = max_value[2], max_value[3], max_value[4]
    x_max = max(25920, max_value[5])
    y_max = max(19440, max_value[6])
    count_max = min(100, max_value[8])
    scale, gap, margin = 0.01, 0.1, 50
    width = int((swath_max * x_max * (1.0 + gap)) * scale + 2 * margin)
    height = int((tile_max * y_max * (1.0 + gap)) * scale + 2 * margin)
    size = width * height
    pixels = [dict() for _ in range(camera_max + 1)]
    counts = [0] * (camera_max + 1)
    for r in records:
        surface, swath, camera, tile, x, y, base, count = r[1:9]
        counts[camera] += 1
        alpha = float(count) / float(count_max)
        blend = COLORS[base]
        px = int(((swath - 1) * (1.0 + gap) * x_max + x) * scale + margin)
        py = int(((tile - 1) * (1.0 + gap) * y_max + y) * scale + margin)
        off = py * width + px
        if off >= size or off < -size:
            return False
        off %= size
        pix = pixels[camera].get(off, (0, 0, 0))
        pixels[camera][off] = tuple(min(255, int(alpha * blend[c] + (1.0 - alpha) * pix[c])) for c in range(3))
    for camera in range(camera_max + 1):
        if counts[camera] == 0:
            continue
        buf = np.zeros((size, 3), dtype=np.uint8)
        if pixels[camera]:
            offs = np.fromiter(pixels[camera].keys(), dtype=np.int64, count=len(pixels[camera]))
            buf[offs] = np.clip(np.array(list(pixels[camera].values()), dtype=np.int64), 0, 255)
        img = Image.fromarray(buf.reshape(height, width, 3), "RGB")
        img.save(os.path.join(output, "image_by_camera", str(lane) + "_" + str(camera) + ".png"))
        print("finished drawing lane " + str(lane) + " camera: " + str(camera))
    return True


def process_records(records, output, draw):
    """BubbleProcesser.run after the merge: returns the circles (always none: see the module docstring)"""
    print("finished polyX stat for all files")
    if records:
        xmax = max(max(r[5] for r in records), 0)
        ymax = max(max(r[6] for r in records), 0)
    else:
        xmax = ymax = 0
    records.sort(key=lambda r: r[1])
    records.sort(key=lambda r: r[9] % 10000)
    records.sort(key=lambda r: r[0])
    print("write records to poly_X.csv")
    if not os.path.exists(output):
        os.makedirs(output)
    write_records(os.path.join(output, "poly_X.csv"), records)
    print("process records by tile")
    by_tile = os.path.join(output, "record_by_tile")
    if not os.path.exists(by_tile):
        os.makedirs(by_tile)

    def flush(group, tile_no, lane):
        write_records(os.path.join(by_tile, str(lane) + "_x" + str(tile_no) + ".csv"), group)
        if not os.path.exists(os.path.join(output, "image_by_tile")):
            os.makedirs(os.path.join(output, "image_by_tile"))
        if detect_tile(group, xmax, ymax):
            raise ZeroDivisionError("float division by zero (CircleDetector.detectDirectly: the detector's record list "
                                    "is emptied in its __init__, circledetector.py:19)")

    group, last_tile, last_lane = [], -1, -1
    for r in records:
        tile_no = r[9] % 10000
        if tile_no != last_tile:
            if last_tile != -1:
                flush(group, last_tile, last_lane)
                group = []
            last_tile = tile_no
        if r[0] != last_lane:
            last_lane = r[0]
        group.append(r)
    if last_tile != -1:
        flush(group, last_tile, last_lane)
    if draw:
        print("draw images")
        cam_dir = os.path.join(output, "image_by_camera")
        if not os.path.exists(cam_dir):
            os.makedirs(cam_dir)
        if records:
            try:
                from PIL import Image
            except ImportError:
                Image = None
                print("PIL is not importable: the image_by_camera maps are skipped")
            if Image is not None:
                max_value = [0] * 10
                for r in records:
                    for i in range(10):
                        max_value[i] = max(max_value[i], r[i])
                lanes = {}
                for r in records:
                    lanes.setdefault(r[0], []).append(r)
                for lane in sorted(lanes):                  # lanes without records: upstream's child dies, no image
                    draw_lane(lanes[lane], max_value, output, Image)
    return []


def list_fastqs(folder):
    """debubbleDir's file list (debubble.py:16-24): os.listdir order, files only, fastq.isFastq"""
    out = []
    for f in os.listdir(folder):
        path = os.path.join(folder, f)
        if os.path.isdir(path):
            continue
        if fastq.isFastq(path):
            out.append(path)
    return out


def write_circles(circles, outdir):
    """debubble.writeCircles (debubble.py:6-15)"""
    if not os.path.exists(outdir):
        return
    with open(os.path.join(outdir, "circles.csv"), "w") as f:
        f.write("x,y,radius,lane,tile\n")
        for c in circles:
            f.write("%s,%s,%s,%s,%s\n" % (c[0], c[1], c[2], c[4], c[5]))


def debubbleDir(folder, poly_max, output, draw, engine=None):
    """debubble.debubbleDir (debubble.py:18-35).  engine: see census_files"""
    if engine is None:
        engine = os.environ.get("AQC_DEBUBBLE_ENGINE") or None       # "host": census_host (machines without a GPU)
    files = list_fastqs(folder)
    circles = []
    if not files:
        print("No fastq files")
    else:
        per_file = census_files(files, poly_max, engine)
        records = []
        for r in per_file:
            records += r
        circles = process_records(records, output, draw)
    if circles:
        print("detected bubbles:")
        print(circles)
    else:
        print("no bubble detected")
    write_circles(circles, output)
    return circles


def parseCommand(argv=None):
    """debubble.py:10-22"""
    parser = OptionParser(usage="usage: %prog <input_files> [options]", version="%prog 1.1")
    parser.add_option("-p", "--poly_max", dest="poly_max", default=20, type="int", help="Min polyX to draw on tile images. Default is 20.")
    parser.add_option("-o", "--output", dest="output", default="bubble", help="folder to store the csv and image files. Default is bubble.")
    parser.add_option("-i", "--input", dest="input", default=".", help="folder storing input fastq files. Default is current dir.")
    parser.add_option("-d", "--draw", dest="draw", default="on", help="specify whether draw the pictures or not. Default is on.")
    return parser.parse_args(argv)


def main(argv=None):
    """runInFolder (debubble.py:37-45)"""
    from .after import parseBool
    t0 = time.time()
    options, _ = parseCommand(argv)
    debubbleDir(options.input, options.poly_max, options.output, parseBool(options.draw))
    print('Time used in folder: ' + str(time.time() - t0))


if __name__ == "__main__":
    main()
