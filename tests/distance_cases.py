"""The distance mode's row rules restated in plain Python (reference console_distance.cpp:58-204, the product's host loop in host/main.cpp):
the witness the device path is compared with.  Values come from kmdbh_metric over ctypes (the reference's arithmetic, libm's log), the text
of a value from int(v * 1e6 + 0.5).  Nothing here goes through kmdb_distance_* or kmdbh_format_measure."""
import ctypes
import re

import numpy as np

M32 = 0xFFFFFFFF
DBL_MAX = float(np.finfo(np.float64).max)
METRICS = ["jaccard", "min", "max", "cosine", "mash", "ani", "ani-shorter", "mash-query", "num-kmers"]


def to_u64(t):
    """(unsigned long long) of a double as x86-64 converts it: below 2^63 one cvttsd2si; from 2^63 on the same of t - 2^63 with the top bit set;
    what the instruction cannot represent (NaN, infinities) is its 'integer indefinite' 2^63"""
    if t != t:
        return 1 << 63
    if t < 2.0 ** 63:
        return int(t)
    u = t - 2.0 ** 63
    return (int(u) | (1 << 63)) if u < 2.0 ** 63 else 0


def fmt_measure(v):
    """Double2PChar with six decimals as the console prints a measure (conversion.h:167-219, 262-268)"""
    if v == 0:
        return b"0"
    sign = b""
    if v < 0:
        sign, v = b"-", -v
    x = to_u64(v * 1000000.0 + 0.5)
    return sign + b"%d.%06d" % (x // 1000000, x % 1000000)


class Rules:
    """One run of the loop: the state it carries from row to row (sparse output once a pair was met, the triangle) and what it was started with."""

    def __init__(self, L, measure, k, counts, bounds=(), kmer_lo=0, kmer_hi=M32, sparse_out=False, phylip=False, triangle=False, names=None, cache=None):
        self.L, self.measure, self.k = L, METRICS.index(measure), int(k)
        self.counts = [int(c) & M32 for c in counts]
        self.bounds = [(METRICS.index(m), -DBL_MAX if lo is None else lo, DBL_MAX if hi is None else hi) for m, lo, hi in bounds]
        self.kmer_lo, self.kmer_hi = kmer_lo, kmer_hi
        self.phylip = phylip
        self.sparse_out = sparse_out and not phylip
        self.triangle = triangle
        self.cache = {} if cache is None else cache      # kmdbh_metric's values, shared between runs over the same table
        self.names = names                       # the header's sample names: row 0 decides the triangle; None: the caller has decided

    def metric(self, m, c, a, b):
        key = (m, c, a, b)
        v = self.cache.get(key)
        if v is None:
            v = self.cache[key] = self.L.kmdbh_metric(m, ctypes.c_uint32(c), ctypes.c_uint32(a), ctypes.c_uint32(b), self.k)
        return v

    def passes(self, common, a, col):
        for m, lo, hi in self.bounds:
            x = self.metric(m, common, a, self.counts[col])
            if not (x >= lo and x <= hi):
                return False
        return self.kmer_lo <= common <= self.kmer_hi

    def row(self, line, row):
        n = len(self.counts)
        s = line + b"\0"
        end = len(line)
        comma = line.find(b",")
        comma = end if comma < 0 else comma
        qname = line[:comma]
        p = comma + 1 if comma < end else end

        def read_uint(p):
            v = 0
            while 48 <= s[p] <= 57:
                v = v * 10 + s[p] - 48
                p += 1
            return v & 0xFFFFFFFFFFFFFFFF, p
        a, p = read_uint(p)
        a &= M32
        if p < end:
            p += 1
        dense, hits, n_read = [0] * n, [], 0
        while end - p > 1:
            v, p = read_uint(p)
            if s[p] == 58:                       # ':' — a pair: 1-based column, count
                common, p = read_uint(p + 1)
                common &= M32
                if self.phylip:
                    if 1 <= v <= n:
                        dense[v - 1] = common
                else:
                    self.sparse_out = True
                    if common > 0 and 1 <= v <= n and self.passes(common, a, v - 1):
                        hits.append((v - 1, common))
            elif self.sparse_out:
                if v > 0 and n_read < n and self.passes(v & M32, a, n_read):
                    hits.append((n_read, v & M32))
            elif n_read < n:
                dense[n_read] = v & M32
            if p < end:
                p += 1
            n_read += 1
        if self.names is not None and row == 0:
            empty_first = (not hits) if self.sparse_out else (n == 0 or dense[0] == 0)
            if self.names and qname == self.names[0] and empty_first:
                self.triangle = True
        n_proc = len(hits) if self.sparse_out else (min(row, n) if self.triangle else n)
        out = [qname]
        if self.phylip:
            out.append(b" ")
            for c in range(min(n_read, n)):
                out.append(fmt_measure(self.metric(self.measure, dense[c], a, self.counts[c]) if c < n_proc else 0.0) + b" ")
        else:
            out.append(b",")
            if self.sparse_out:
                for col, common in hits:
                    out.append(b"%d:" % (col + 1) + fmt_measure(self.metric(self.measure, common, a, self.counts[col])) + b",")
            else:
                for c in range(n_proc):
                    out.append(fmt_measure(self.metric(self.measure, dense[c], a, self.counts[c])) + b",")
        out.append(b"\n")
        return b"".join(out)

    def rows(self, text, first_row=0):
        """a run of whole rows, as getline cuts them"""
        lines = text.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        return b"".join(self.row(ln, first_row + i) for i, ln in enumerate(lines))


def parse_options(opts):
    """the front-end's reading of the distance arguments (params.cpp:603-668) -> keyword arguments of Rules and the measure"""
    opts = list(opts)
    kw = {"sparse_out": "-sparse" in opts, "phylip": "-phylip-out" in opts}
    opts = [o for o in opts if o not in ("-sparse", "-phylip-out")]
    lo_hi = {}
    kmer = [0, M32]
    rest = []
    i = 0
    while i < len(opts):
        if opts[i] in ("-min", "-max"):
            which = 0 if opts[i] == "-min" else 1
            crit, _, num = opts[i + 1].rpartition(":")
            crit = crit if _ else "?"
            if crit == "num-kmers":
                kmer[which] = int(round(float(num)))
            else:
                lo_hi.setdefault(crit, [None, None])[which] = float(num)
            i += 2
        else:
            rest.append(opts[i])
            i += 1
    measure = rest[0]
    if "?" in lo_hi:
        lo_hi[measure] = lo_hi.pop("?")
    kw["bounds"] = [(m, lo, hi) for m, (lo, hi) in sorted(lo_hi.items())]
    kw["kmer_lo"], kw["kmer_hi"] = kmer
    return measure, kw


def parse_table(data):
    """-> k, the fraction as text, the header's rest, the names, the counts, the body"""
    line1, line2, body = (data.split(b"\n", 2) + [b"", b""])[:3]
    m = re.match(rb"\s*\S+\s+(\d+)\s+\S+\s+(\S+)\s+\S+(.*)$", line1, re.S)      # in >> tok >> k >> tok >> fraction >> tok; getline(rest)
    k, fraction, rest = int(m.group(1)), float(m.group(2)), m.group(3)
    names = rest.replace(b",", b" ").split()
    counts = []
    for w in line2.replace(b",", b" ").split()[2:]:
        if not w.isdigit():
            break
        counts.append(int(w) & M32)
    return k, fraction, rest, names, counts, body


def distance_file(L, data, opts):
    """the whole mode on a table's bytes: header lines and every row"""
    measure, kw = parse_options(opts)
    k, fraction, rest, names, counts, body = parse_table(data)
    out = []
    if not kw["phylip"]:
        out.append(b"kmer-length: %d fraction: %s" % (k, ("%g" % fraction).encode()) + rest + b"\n")
    else:
        out.append(b"%d\n" % len(counts))
    r = Rules(L, measure, k, counts, names=names, **kw)
    out.append(r.rows(body))
    return b"".join(out)


# ---- tables for the device tests -----------------------------------------------------------------------------------------------------------
def header(k, names, counts):
    return (b"kmer-length: %d fraction: 1 ,db-samples ," % k + b"".join(n + b"," for n in names) + b"\n"
            + b"query-samples,total-kmers," + b"".join(b"%d," % c for c in counts) + b"\n")


def random_counts(rng, n):
    return rng.integers(3_000_000, 6_000_000, n).astype(np.int64)


def dense_body(names, row_counts, cells, triangle=False):
    """cells[r][c]; a triangle keeps c < r"""
    out = []
    for r, nm in enumerate(names):
        row = cells[r][:r] if triangle else cells[r]
        out.append(nm + b",%d," % row_counts[r] + b"".join(b"%d," % v for v in row) + b"\n")
    return b"".join(out)


def sparse_body(names, row_counts, cells, triangle=False):
    out = []
    for r, nm in enumerate(names):
        row = cells[r][:r] if triangle else cells[r]
        out.append(nm + b",%d," % row_counts[r] + b"".join(b"%d:%d," % (c + 1, v) for c, v in enumerate(row) if v) + b"\n")
    return b"".join(out)
