#!/usr/bin/env python3
"""Record what the REAL reference makes of read names of every shape, for tests/test_writer_cases_cpu.py:

  * barcodeprocesser.moveBarcodeToName (barcodeprocesser.py:34-45) of [name, read, '+', qual] — the name becomes
    '@' + barcode + name[name.find(':'):], and find() == -1 slices the last character — for the names of
    writer_cases.barcode_name_list() and one read each of 17, 18, 30 and 60 bases (12 barcode bases + CAGTA + the rest);
  * the bad-record rename of seqFilter.writeReads (preprocesser.py:206-232): '@' + FLAG + name[1:].

Writes tests/golden/writer_names.json.gz: data only.  Run where the reference is present (the py3 shim is make_golden's)."""
import gzip
import json
import os
import random
import sys

import make_golden
from make_golden import HERE, REF, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

READ_LENGTHS = (17, 18, 30, 60)
FLAGS = ("BADBCD1", "BADLEN", "BADMISMATCH")


class Sink:
    def __init__(self):
        self.lines = []

    def writeLines(self, lines):
        self.lines.append(list(lines))


class Options:
    qc_only = False


class Holder:
    options = Options()


def main():
    if not os.path.isdir(REF):
        print("reference not present at %s: the fixture can only be regenerated where it is" % REF)
        sys.exit(2)
    make_golden.install_shim()
    import barcodeprocesser
    import preprocesser
    import writer_cases
    rng = random.Random(20261020)
    # one read per length (the names are what varies), a quality line that says where each character stood
    reads = {}
    for L in READ_LENGTHS:
        read = "".join(rng.choice("ACGT") for _ in range(12)) + "CAGTA" + "".join(rng.choice("ACGT") for _ in range(L - 17))
        reads[str(L)] = {"read": read, "qual": "".join(chr(53 + (3 * i) % 20) for i in range(L))}
    names = []
    for cls, name in writer_cases.barcode_name_list():
        name = name.decode("latin-1")
        moved = {}
        for L, rd in reads.items():
            rec = [name, rd["read"], "+", rd["qual"]]
            barcodeprocesser.moveBarcodeToName(rec, 12, "CAGTA")
            moved[L] = [rec[0], rec[1], rec[3]]
        renamed = {}
        for flag in FLAGS:
            sink = Sink()
            rd = reads[str(READ_LENGTHS[0])]
            preprocesser.seqFilter.writeReads(Holder(), [name, rd["read"], "+", rd["qual"]], None, None, None, sink, None, None, None, flag)
            renamed[flag] = sink.lines[0][0]
        names.append({"class": cls, "name": name, "moved": moved, "renamed": renamed})
    out = {"reads": reads, "names": names}
    path = os.path.join(HERE, "writer_names.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    print("wrote %s: %d names, %d bytes" % (path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
