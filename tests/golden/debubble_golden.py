"""The debubble golden cases (debubble_cases.json.gz, written by make_debubble.py from the reference): load them, lay a
case's input folder out on disk, and gather an output folder in the form the fixture keeps."""
import bz2
import gzip
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cases():
    with gzip.open(os.path.join(HERE, "debubble_cases.json.gz"), "rt") as f:
        return json.load(f)


def write_inputs(folder, files):
    os.makedirs(folder, exist_ok=True)
    for fn, text in files.items():
        p = os.path.join(folder, fn)
        if fn.endswith(".gz"):
            with gzip.open(p, "wb") as f:
                f.write(text.encode())
        elif fn.endswith(".bz2"):
            with bz2.open(p, "wb") as f:
                f.write(text.encode())
        else:
            with open(p, "w") as f:
                f.write(text)


def outputs(out):
    """{dirs, files: text of every non-image file, images: size + sha256 of the decoded RGB pixels}"""
    from PIL import Image
    res = dict(dirs=[], files={}, images={})
    if not os.path.exists(out):
        return res
    for root, dirs, files in os.walk(out):
        rel = os.path.relpath(root, out)
        for d in dirs:
            res["dirs"].append(os.path.normpath(os.path.join(rel, d)))
        for f in files:
            p = os.path.join(root, f)
            k = os.path.normpath(os.path.join(rel, f))
            if f.endswith(".png"):
                im = Image.open(p).convert("RGB")
                res["images"][k] = dict(size=list(im.size), sha256=hashlib.sha256(im.tobytes()).hexdigest())
            else:
                with open(p) as fh:
                    res["files"][k] = fh.read()
    res["dirs"].sort()
    return res


def check(got, expect, exception):
    """the pass's outputs and outcome against the reference's"""
    assert exception == expect["exception"]
    assert got["dirs"] == expect["dirs"]
    assert sorted(got["files"]) == sorted(expect["files"])
    for k, text in expect["files"].items():
        assert got["files"][k] == text, k
    assert got["images"] == expect["images"]
    assert ("circles.csv" in got["files"]) == expect["circles"]


def run_case(case, tmp, engine):
    """debubbleDir over the case's folder the way after.runDebubble calls it, files in sorted order; returns (outputs,
    exception type name)"""
    from afterqc_amd import debubble
    folder = os.path.join(str(tmp), "in")
    write_inputs(folder, case["files"])
    out = os.path.join(str(tmp), "debubble")
    err = None
    listing = debubble.list_fastqs
    debubble.list_fastqs = lambda f: sorted(listing(f))      # the fixture's listing order (make_debubble.py)
    try:
        debubble.debubbleDir(folder, 20, out, case["draw"], engine=engine)
    except Exception as e:
        err = type(e).__name__
    finally:
        debubble.list_fastqs = listing
    return outputs(out), err
