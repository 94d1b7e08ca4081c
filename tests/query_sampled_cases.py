"""Inputs and references of test_new2all_sampled.py: rectangles of QUERY rows crafted cell by cell for kmdb_sampled_from_rows_device, placed on
the constants of the row-segment source of csrc/sample_rows.hip — lines of 64 cells, segments of 2048 columns, a flat range [cell_lo, cell_hi)
that cuts rows and segments — and on those of the select itself (the four digits, the float key, unrankable cells, the margin band).  Host only.

The reference is never the device.  It is expected_rows: the rule of `new2all -sample-rows` restated in numpy over the cells of the range —
the non-zero cells that pass the exact bounds, scored by kmdbh_metric with a = the QUERY's k-mer count and b = the database sample's, per query
the `count` best by (score descending, sample id ascending), listed in ascending id.  One-sided: the samples collect nothing.  A NaN score
ranks below every number (host_sampler.cpp's better())."""
import numpy as np

from parts_sampled_cases import WIDEN, exact_pass, widened_pass  # noqa: F401  (the tests import them from here)
from sample_rows_cases import BAND_HI, KEY_BEST, K_LEN, count_inside_key, key_of, settle_digit  # noqa: F401
from test_sample_rows_device import CRITERIA, metric_of, proxy_of  # noqa: F401

SEG = 2048                                              # N2S_SEG: columns per segment, a wave each
WIDTHS = (1, 63, 64, 65, 2047, 2048, 2049, 4097)


class Rows:
    """one nq x nc rectangle of query rows, the queries' counts a, the samples' counts b and the calls (criterion, count, filters) made on it"""

    def __init__(self, name, nq, nc, a, b, runs=()):
        self.name, self.nq, self.nc, self.runs = name, nq, nc, list(runs)
        self.a = np.broadcast_to(np.asarray(a, np.int64), (nq,)).copy()
        self.b = np.broadcast_to(np.asarray(b, np.int64), (nc,)).copy()
        self.dense = np.zeros((nq, nc), np.uint32)
        self.rng = np.random.default_rng(sum(name.encode()))
        self._expected = {}

    def put(self, q, s, v):
        assert self.dense[q, s] == 0 and 0 < v < 1 << 32
        self.dense[q, s] = v

    def fill(self, density, lo, hi):
        m = (self.rng.random((self.nq, self.nc)) < density) & (self.dense == 0)
        self.dense[m] = self.rng.integers(lo, hi + 1, (self.nq, self.nc))[m]
        return self

    def line(self, q, values, avoid=()):
        """`values` on distinct random columns of row q (not in `avoid`): the columns spread over every segment of the row"""
        cols = self.rng.permutation(np.setdiff1d(np.arange(self.nc), avoid))[:len(values)]
        assert len(cols) == len(values)
        for s, v in zip(cols.tolist(), values):
            self.put(q, s, int(v))
        return cols

    def triplets(self, lo=0, hi=None):
        """(q, s, v) of the non-zero cells of the flat range [lo, hi), row-major"""
        q, s = np.nonzero(self.dense)
        flat = q.astype(np.int64) * self.nc + s
        m = (flat >= lo) & (flat < (self.nq * self.nc if hi is None else hi))
        return q[m].astype(np.int64), s[m].astype(np.int64), self.dense[q[m], s[m]].astype(np.int64)


def expected_rows(K, case, criterion, count, filters=(), lo=0, hi=None, k=K_LEN):
    """the rule over the cells of the range: nq rows of (sample id, value), ascending ids"""
    key = (criterion, count, tuple(filters), lo, hi)
    if key not in case._expected:
        q, s, v = case.triplets(lo, hi)
        ok = exact_pass(K, q, s, v, case.a, case.b, k, filters)
        q, s, v = q[ok], s[ok], v[ok]
        sc = metric_of(K, criterion, v, case.a[q], case.b[s], k)
        per = [[] for _ in range(case.nq)]
        for qq, ss, vv, x in zip(q.tolist(), s.tolist(), v.tolist(), sc.tolist()):
            nan = x != x
            per[qq].append((nan, 0.0 if nan else -x, ss, vv))
        case._expected[key] = [sorted((o, x) for _, _, o, x in sorted(row)[:count]) for row in per]
    return case._expected[key]


def widened_rows(case, filters=(), lo=0, hi=None):
    """per query the samples whose cell the device may emit: not zero, inside the range and inside every widened bound"""
    q, s, v = case.triplets(lo, hi)
    ok = widened_pass(q, s, v, case.a, case.b, filters)
    out = [set() for _ in range(case.nq)]
    for qq, ss in zip(q[ok].tolist(), s[ok].tolist()):
        out[qq].add(ss)
    return out


def row_proxies(case, criterion, q):
    s = np.flatnonzero(case.dense[q])
    return proxy_of(criterion, case.dense[q, s].astype(np.int64), np.full(len(s), case.a[q]), case.b[s])


def band_is_empty(case, criterion, count, q):
    """no cell of row q below its count-th best proxy T lies within the margin band of T — and no other cell shares T's float key: the device must
    emit exactly `count` cells of the row"""
    p = np.sort(row_proxies(case, criterion, q))[::-1]
    assert len(p) > count
    T = p[count - 1]
    return bool(p[count] < T - abs(T) * BAND_HI and key_of(p[count:count + 1])[0] != key_of(p[count - 1:count])[0])


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------
def width_case(nq, nc):
    """half of the cells set; the queries' counts from another range than the samples'; counts 1, 5, the row exactly and one larger than the row"""
    c = Rows("width_%dx%d" % (nq, nc), nq, nc, 0, 0)
    c.a = 6000 + c.rng.integers(0, 3000, nq)
    c.b = 9000 + c.rng.integers(0, 9000, nc)
    c.fill(0.5, 1, 5000)
    if not c.dense[nq - 1, nc - 1]:
        c.put(nq - 1, nc - 1, 17)                       # the last cell of the last line of the last segment
    exactly = int(np.count_nonzero(c.dense[0])) or 1
    c.runs = [("jaccard", n, ()) for n in sorted({1, 5, exactly, nc + 7})] + [("num-kmers", 5, ())]
    if (nq, nc) == (3, 2049):
        c.runs += [(cr, 5, ()) for cr in CRITERIA if cr not in ("jaccard", "num-kmers")]
    return c


DIGIT_NQ, DIGIT_NC = 3, 2500                            # two segments, the second of 452 columns (a last line of 4)
DIGIT_VALUES = {
    "digit0": (4 ** np.arange(16), 5, 0),
    "digit1": (65536 * (1 + np.arange(100)), 40, 1),
    "digit2": (256 + np.arange(256), 100, 2),
    "digit3": ((1 << 23) + np.arange(256), 100, 3),
}
EXACT = ("digit0", "digit1", "digit2")                  # the cut stands clear of every other cell (census: band_is_empty)
COLLAPSE_VALUES = (1 << 24) + 1 + 2 * np.arange(200)    # 200 cells on 101 float keys


def digit_case(name):
    """num-kmers with every count 1000: the proxy is the cell.  Every row holds `values` on columns of its own choice, over both segments."""
    if name == "collapse":
        values, count = COLLAPSE_VALUES, count_inside_key(key_of(COLLAPSE_VALUES), 50)
    else:
        values, count, _ = DIGIT_VALUES[name]
    c = Rows(name, DIGIT_NQ, DIGIT_NC, 1000, 1000, [("num-kmers", count, ())])
    for q in range(DIGIT_NQ):
        cols = c.line(q, values)
        assert cols.min() < SEG <= cols.max()
    return c


def unrankable_case():
    """row 0: a sample of k-mer count 0 (min(a, 0) = 0: the proxy of min, ani-shorter and cosine is infinite); row 1: a cell c = a + b (the jaccard
    denominator a + b - c wraps to 0); row 2: 60 rankable cells; row 3: a query count of 0 (mash-query and min divide by it).  Rows that hold a
    cell the device cannot rank come out whole, the others are cut."""
    c = Rows("unrankable", 4, 300, 0, 0)
    c.a = np.array([2000, 2100, 2200, 0])
    c.b = 3000 + c.rng.integers(0, 500, 300)
    c.b[70] = 0
    c.put(0, 70, 50)
    c.put(1, 131, int(c.a[1] + c.b[131]))
    c.fill(0.2, 1, 1500)
    c.dense[1:, 70] = 0                                 # (the sample of count 0 stands beside row 0 alone)
    c.runs = [(cr, 2, ()) for cr in ("min", "ani-shorter", "cosine", "jaccard", "mash-query", "num-kmers")]
    return c


def unrankable_rows(case, criterion):
    return {q for q in range(case.nq) if (key_of(row_proxies(case, criterion, q)) == KEY_BEST).any()}


def tied_case():
    """row 1 of a 2 x 4097 rectangle holds 1 500 cells of value 7 (every count 1000): one key in all four passes, everything is a candidate, the
    host keeps the five lowest ids; row 0 holds 3 cells"""
    c = Rows("tied", 2, 4097, 1000, 1000, [("num-kmers", 5, ()), ("jaccard", 5, ())])
    c.line(1, [7] * 1500)
    c.line(0, [9, 8, 7])
    return c


def refetch_case():
    """num-kmers:3 under -min jaccard.  Query 1 (count 1000): its three largest cells are 600, 550 and X = 500, X beside sample 200 of count 10 000 —
    jaccard 500 / 10 500, the smallest of the rectangle; the bound is one ulp above it, so X passes the widened bound, fails the exact one, and
    the row has two exact passes at or above its cut: it is fetched again, and the cell that takes X's place (400) lay below the cut.  Every
    other cell has counts 1000 / 1000 and a value >= 100: jaccard >= 100 / 1900."""
    c = Rows("refetch", 3, 2100, 1000, 1000)
    c.b[200] = 10_000
    c.put(1, 200, 500)
    for s, v in zip((5, 64, 130, 2050, 66, 2099), (600, 550, 400, 300, 200, 100)):
        c.put(1, s, v)
    for q in (0, 2):                                    # 300 distinct values: the cut of these rows stands clear of every other cell
        c.line(q, 100 + np.arange(300), avoid=(200,))
    bound = float(np.nextafter(500.0 / 10_500.0, 2.0))
    c.runs = [("num-kmers", 3, (("jaccard", bound, None),))]
    return c


def zero_case():
    """row 1 is zero; rows 0 and 2 hold 30 cells"""
    c = Rows("zero", 3, 130, 5000, 7000, [("jaccard", 4, ()), ("mash-query", 4, ())])
    c.a = np.array([5000, 5100, 5200])
    c.line(0, 100 + 13 * np.arange(30))
    c.line(2, 100 + 17 * np.arange(30))
    return c


BIG_NQ, BIG_NC = 70_000, 70_001                         # the last rows start beyond 2^32 cells
assert (BIG_NQ - 3) * BIG_NC > 1 << 32


def big_case():
    """the LAST THREE rows of a 70 000 x 70 001 rectangle as a rectangle of their own (the test passes them as the flat range
    [(nq - 3) * n_cols, nq * n_cols) of the large one): cells on both sides of every segment border and in the last line"""
    c = Rows("big", 3, BIG_NC, 0, 0, [("jaccard", 4, ()), ("jaccard", 40, ())])
    c.a = np.array([5000, 6000, 7000])
    c.b = 7000 + np.arange(BIG_NC) % 991
    for q in range(3):
        for x, s in enumerate((0, 63, 64, 2047, 2048, 4095, 4096, 33_000, 65_535, 65_536, 69_999, 70_000)):
            c.put(q, s, 100 + 37 * x + 500 * q)
    return c


_CASES = {}


def case(name):
    if name not in _CASES:
        if name.startswith("width_"):
            nq, nc = (int(x) for x in name[6:].split("x"))
            _CASES[name] = width_case(nq, nc)
        elif name in DIGIT_VALUES or name == "collapse":
            _CASES[name] = digit_case(name)
        else:
            _CASES[name] = {"unrankable": unrankable_case, "tied": tied_case, "refetch": refetch_case, "zero": zero_case, "big": big_case}[name]()
    return _CASES[name]


WIDTH_NAMES = ["width_%dx%d" % (nq, nc) for nc in WIDTHS for nq in (1, 3)]
DIGIT_NAMES = list(DIGIT_VALUES) + ["collapse"]

# flat ranges of the 3 x 4097 rectangle: whole; cut in the middle of row 1; cut on a segment border of row 0; one cell past it; inside one segment of
# row 1; empty; from the middle of row 0's second segment to the middle of row 2
RANGE_NC = 4097
RANGES = [(0, 3 * RANGE_NC), (0, RANGE_NC + 1000), (0, SEG), (0, SEG + 1), (RANGE_NC + 2100, RANGE_NC + 2200), (5, 5), (3000, 2 * RANGE_NC + 3000)]
SPLIT = RANGE_NC + 2048 + 700                           # two consecutive ranges [0, SPLIT), [SPLIT, end): the cut inside row 1's second segment
