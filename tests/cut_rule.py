"""The specification of per-read sliding-window quality cutting (--cut_front / --cut_tail / --cut_right), as plain python.

The cut stands inside the trim stage of preprocesser.py:455-466, behind upstream's fixed trim.  Every quality byte counts as
byte - 33 (util.qualNum; any byte value, negative results included), a window is good when its integer sum reaches Q * w.
cut_window is the model; precut turns a record into the record a run WITHOUT the options would have to be given to write the same
reads; the rest are the helpers the tests share (a brute-force restatement, the counts of aqc_get_cut_stats, seeded inputs)."""
import random


class CutConfig:
    def __init__(self, front=False, tail=False, right=False, window=4, mean_quality=20, trim_front=0, trim_tail=0, trim_front2=None, trim_tail2=None):
        self.front, self.tail, self.right = bool(front), bool(tail), bool(right)
        self.window, self.mean_quality = int(window), int(mean_quality)
        self.trim_front, self.trim_tail = int(trim_front), int(trim_tail)
        self.trim_front2 = self.trim_front if trim_front2 is None else int(trim_front2)
        self.trim_tail2 = self.trim_tail if trim_tail2 is None else int(trim_tail2)

    @property
    def on(self):
        return self.front or self.tail or self.right

    def modes(self):
        return self.front, self.tail, self.right


MODES = [(f, t, r) for f in (0, 1) for t in (0, 1) for r in (0, 1) if f or t or r]      # the seven combinations


def trim(s, front, tail):
    """preprocesser.py:19-28"""
    if tail > 0:
        return s[front:-tail]
    return s[front:]


def cut_window(q, W, Q, front, tail, right):
    """q: the quality BYTES of one read after trim(); -> (c0, c1), keep [c0:c1]"""
    n = len(q)
    if n == 0: return 0, 0
    w = min(W, n)                                   # a read shorter than the window is one window
    P = [0]
    for b in q: P.append(P[-1] + b - 33)
    good = [P[i + w] - P[i] >= Q * w for i in range(n - w + 1)]     # integers only, no mean, no float
    if (front or tail) and not any(good): return 0, 0
    c0 = good.index(True) if front else 0
    c1 = (len(good) - 1 - good[::-1].index(True)) + w if tail else n
    if right:
        bad = [i for i in range(c0, len(good)) if not good[i]]
        if bad: c1 = min(c1, bad[0])
    return c0, max(c1, c0)


def cut_window_brute(q, W, Q, front, tail, right):
    """the same rule restated with direct window sums and explicit scans"""
    n = len(q)
    if n == 0:
        return 0, 0
    w = W if W < n else n
    good = []
    for i in range(n - w + 1):
        total = 0
        for j in range(i, i + w):
            total += q[j] - 33
        good.append(total >= Q * w)
    first = last = None
    for i, g in enumerate(good):
        if g:
            if first is None:
                first = i
            last = i
    if (front or tail) and first is None:
        return 0, 0
    c0 = first if front else 0
    c1 = last + w if tail else n
    if right:
        for i in range(c0, len(good)):
            if not good[i]:
                if i < c1:
                    c1 = i
                break
    return c0, (c1 if c1 > c0 else c0)


def cut_lines(s, q, cfg, mate=0):
    """the sequence and quality line of one mate (bytes) as the trim stage with the cut leaves them"""
    tf, tt = (cfg.trim_front, cfg.trim_tail) if mate == 0 else (cfg.trim_front2, cfg.trim_tail2)
    s1, q1 = trim(s, tf, tt), trim(q, tf, tt)
    c0, c1 = cut_window(q1, cfg.window, cfg.mean_quality, *cfg.modes()) if cfg.on else (0, len(q1))
    return s1[c0:c1], q1[c0:c1]


def precut(record, cfg, mate=0):
    """record: (name, seq, strand, qual) as bytes -> the record with line 2 = trim(s)[c0:c1], line 4 = trim(q)[c0:c1]"""
    name, s, strand, q = record
    s2, q2 = cut_lines(s, q, cfg, mate)
    return name, s2, strand, q2


def cut_counts(pairs, cfg, accum_limit=None):
    """aqc_get_cut_stats of a run over `pairs` ((s1, q1, s2, q2) bytes; s2 None: single-end): reads of R1 the cut made shorter,
    bases it removed from them, the same for R2 — R2 only where read 1 kept 5 bases or more (no BADTRIM1)"""
    out = [0, 0, 0, 0]
    for i, (s1, q1, s2, q2) in enumerate(pairs):
        if accum_limit is not None and i >= accum_limit:
            break
        t1 = trim(s1, cfg.trim_front, cfg.trim_tail)
        k1, _ = cut_lines(s1, q1, cfg, 0)
        if len(k1) < len(t1):
            out[0] += 1
            out[1] += len(t1) - len(k1)
        if s2 is None or len(k1) < 5:
            continue
        t2 = trim(s2, cfg.trim_front2, cfg.trim_tail2)
        k2, _ = cut_lines(s2, q2, cfg, 1)
        if len(k2) < len(t2):
            out[2] += 1
            out[3] += len(t2) - len(k2)
    return out


# ---- seeded inputs ------------------------------------------------------------------------------------------------
def decaying_quality(rng, n, good=38, floor=2, knee=None):
    """a quality line that starts high and falls off towards the tail, like a real read's (bytes)"""
    if knee is None:
        knee = rng.randint(n // 3, n) if n else 0
    out = bytearray()
    for i in range(n):
        if i < knee:
            q = good - rng.randint(0, 6)
        else:
            q = max(floor, good - 8 - 3 * (i - knee) // 2 - rng.randint(0, 5))
        out.append(33 + q)
    return bytes(out)


def pattern_lines(n, w, rng):
    """the named quality patterns of the seam test for a line of n bytes and a window of w: (tag, bytes)"""
    hi, lo = 33 + 40, 33 + 2
    out = [("all_good", bytes([hi]) * n), ("all_bad", bytes([lo]) * n)]
    if n:
        ww = min(w, n)
        for start in sorted(set(list(range(0, 34)) + [n - ww])):
            if 0 <= start <= n - ww:
                line = bytearray([lo]) * n
                line[start:start + ww] = bytes([hi]) * ww
                out.append(("one_good_%d" % start, bytes(line)))
        for pos in (15, 16, 17):
            if pos < n:
                line = bytearray([hi]) * n
                line[pos] = lo
                out.append(("one_bad_%d" % pos, bytes(line)))
        line = bytearray([hi]) * n
        line[n - ww:] = bytes([lo]) * ww
        out.append(("bad_end", bytes(line)))
        for tag, byte in (("space", 0x20), ("tab", 0x09), ("del", 0x7f), ("high", 0x80), ("ff", 0xff)):
            line = bytearray(decaying_quality(rng, n))
            for k in range(0, n, 7):
                line[k] = byte
            out.append((tag, bytes(line)))
        out.append(("decay", decaying_quality(rng, n)))
        out.append(("random", bytes(rng.randrange(33, 75) for _ in range(n))))
    return out
