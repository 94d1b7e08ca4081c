"""Inputs and references of test_parts_sampled.py: RECTANGLES of two sample sets crafted cell by cell for kmdb_sampled_from_rect_device, placed
on the constants of the rectangle source of csrc/sample_rows.hip — tiles of 64 x 64 numbered row block * ceil(nc / 64) + column block, a last
column block that is not full (the address of a column >= nc is a cell of the next row), the slots [0, nr) of the row samples and [nr, nr + nc)
of the column samples — and on those of the select itself (the four digits, the float key, unrankable cells, the margin band).  Host only.

The reference is never the device.  It is expected_rect: the sampler's rule restated in numpy over the whole rectangle — the cells that pass the
exact filters, scored by kmdbh_metric with a = the ROW sample's k-mer count and b = the COLUMN sample's, offered to both samples of the pair,
the `count` best by (score descending, id ascending) — in the GLOBAL ids of a two-part collection: the column set is the earlier part (ids
[0, nc)), the row set the later one (ids [nc, nc + nr)), as in a cell of the all2all-parts grid.  With those ids the triangle's row sample (the
larger id) is the rectangle's row sample, so kmdbh_sample_rows_select scores a pair exactly as the cell does."""
import numpy as np

from sample_rows_cases import KEY_BEST, K_LEN, count_inside_key, key_of, settle_digit  # noqa: F401  (the tests import them from here)
from test_sample_rows_device import CRITERIA, FMAX, metric_of, proxy_of  # noqa: F401

WIDEN = 1e-6                                            # the margin of a widened bound (engine.hip: ratio_bound), relative, plus 1e-300
PLAIN = ("jaccard", "min", "max", "cosine", "num-kmers")   # the criteria whose bound is a bound on the plain ratio itself (the cases bound by these only)


class Rect:
    """one rectangle (sparse: the cells that are not zero), the two count arrays and the calls (criterion, count, filters) made on it"""

    def __init__(self, name, nr, nc, row_kmers, col_kmers, runs=()):
        self.name, self.nr, self.nc, self.runs = name, nr, nc, list(runs)
        self.a = np.broadcast_to(np.asarray(row_kmers, np.int64), (nr,)).copy()
        self.b = np.broadcast_to(np.asarray(col_kmers, np.int64), (nc,)).copy()
        self.cells = {}
        self.rng = np.random.default_rng(sum(name.encode()))
        self._expected = {}

    def put(self, r, c, v):
        assert 0 <= r < self.nr and 0 <= c < self.nc and (r, c) not in self.cells and 0 < v < 1 << 32
        self.cells[(r, c)] = int(v)

    def fill(self, density, lo, hi):
        """random cells of value lo .. hi on about `density` of the rectangle (never on a cell that is set)"""
        m = self.rng.random((self.nr, self.nc)) < density
        v = self.rng.integers(lo, hi + 1, (self.nr, self.nc))
        for r, c in zip(*np.nonzero(m)):
            if (int(r), int(c)) not in self.cells:
                self.put(int(r), int(c), int(v[r, c]))
        return self

    def row_line(self, r, values, avoid=()):
        """`values` on distinct columns of row r that are not in `avoid`"""
        cols = self.rng.permutation(np.setdiff1d(np.arange(self.nc), avoid))[:len(values)]
        assert len(cols) == len(values)
        for c, v in zip(cols.tolist(), values):
            self.put(r, c, int(v))

    def col_line(self, c, values, avoid=()):
        rows = self.rng.permutation(np.setdiff1d(np.arange(self.nr), avoid))[:len(values)]
        assert len(rows) == len(values)
        for r, v in zip(rows.tolist(), values):
            self.put(r, c, int(v))

    def triplets(self):
        """(r, c, v) of the non-zero cells in row-major order"""
        if not self.cells:
            z = np.zeros(0, np.int64)
            return z, z, z
        rc = np.array(sorted(self.cells), np.int64)
        return rc[:, 0], rc[:, 1], np.array([self.cells[k] for k in sorted(self.cells)], np.int64)

    def dense(self):
        m = np.zeros((self.nr, self.nc), np.uint32)
        r, c, v = self.triplets()
        m[r, c] = v
        return m

    @property
    def kmers(self):
        """the counts of the two-part collection: the column set first"""
        return np.concatenate([self.b, self.a])


def exact_pass(K, r, c, v, a, b, k, filters):
    ok = np.ones(len(v), bool)
    for name, lo, hi in filters:
        x = metric_of(K, name, v, a[r], b[c], k)
        ok &= (x >= (-FMAX if lo is None else lo)) & (x <= (FMAX if hi is None else hi))
    return ok


def widened_pass(r, c, v, a, b, filters):
    """the cells the device may emit: not zero and inside every bound widened by the margin (bounds on the plain ratios only)"""
    ok = np.ones(len(v), bool)
    for name, lo, hi in filters:
        assert name in PLAIN
        x = proxy_of(name, v, a[r], b[c])
        lo = -np.inf if lo is None else lo - abs(lo) * WIDEN - 1e-300
        hi = np.inf if hi is None else hi + abs(hi) * WIDEN + 1e-300
        ok &= (x >= lo) & (x <= hi)
    return ok


def expected_rect(K, case, criterion, count, filters=(), k=K_LEN):
    """the sampler's rows over the rectangle, in global ids: a list of nc + nr rows of (id, value), ascending ids.  A NaN score ranks below every
    number and among equal scores the smaller id wins (host_sampler.cpp's better())."""
    key = (criterion, count, tuple(filters))
    if key in case._expected:
        return case._expected[key]
    r, c, v = case.triplets()
    ok = exact_pass(K, r, c, v, case.a, case.b, k, filters)
    r, c, v = r[ok], c[ok], v[ok]
    sc = metric_of(K, criterion, v, case.a[r], case.b[c], k)
    per = [[] for _ in range(case.nc + case.nr)]
    for rr, cc, vv, s in zip(r.tolist(), c.tolist(), v.tolist(), sc.tolist()):
        nan = s != s
        per[case.nc + rr].append((nan, 0.0 if nan else -s, cc, vv))
        per[cc].append((nan, 0.0 if nan else -s, case.nc + rr, vv))
    case._expected[key] = [sorted((o, x) for _, _, o, x in sorted(row)[:count]) for row in per]
    return case._expected[key]


def global_part(nr, nc, row_cand, col_cand):
    """the two outputs of a sampled rectangle as ONE candidate part of the two-part collection: rows [0, nc) the column samples (their local row
    ids shifted by nc), rows [nc, nc + nr) the row samples (their local column ids as they are)"""
    rp, cp = row_cand.row_ptr.astype(np.uint64), col_cand.row_ptr.astype(np.uint64)
    assert len(rp) == nr + 1 and len(cp) == nc + 1
    ptr = np.concatenate([cp, cp[-1] + rp[1:]])
    col = np.concatenate([col_cand.col.astype(np.uint32) + np.uint32(nc), row_cand.col.astype(np.uint32)])
    return ptr, col, np.concatenate([col_cand.val, row_cand.val]).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 200), (200, 1), (64, 64), (65, 63), (70, 130), (130, 70)]


def shape_case(nr, nc):
    """half of the cells set, the row samples' counts from another range than the column samples'; counts 1, 5, 64 and one larger than nc"""
    c = Rect("shape_%dx%d" % (nr, nc), nr, nc, 0, 0)
    c.a = 6000 + c.rng.integers(0, 3000, nr)
    c.b = 9000 + c.rng.integers(0, 9000, nc)
    c.fill(0.5, 1, 5000)
    if (nr, nc) == (1, 1):
        c.cells.setdefault((0, 0), 17)
    c.runs = [("jaccard", n, ()) for n in (1, 5, 64, nc + 7)] + [("num-kmers", 5, ())]
    if (nr, nc) == (70, 130):
        c.runs += [(cr, 5, ()) for cr in CRITERIA if cr != "jaccard"] + [("mash-query", 64, ()), ("max", 64, ())]
    return c


def column_edge():
    """nc = 70: the last column block holds columns 64 .. 69 and 58 lanes past the row's end, whose addresses are columns 0 .. 57 of the NEXT row.
    Columns 0 .. 5 of every row hold the largest values of the matrix, descending; columns 64 .. 69 the next largest of the row, descending; the
    rest is small: the best `count` cells of a row are the first `count` of columns 0 .. 5, 64 .. 69.  A lane
    that loaded past nc would hand row r the best cells of row r + 1 under the column ids 70 .. 75."""
    nr, nc = 130, 70
    c = Rect("column_edge", nr, nc, 1000, 1000)
    for r in range(nr):
        for x in range(6):
            c.put(r, x, 1_000_000 + 7 * r + 1000 * (5 - x))          # (steps of 1000 and 100: far outside the 1.5e-6 band of a cut)
            c.put(r, 64 + x, 50_000 + 11 * r + 100 * (5 - x))
        for x in c.rng.choice(np.arange(6, 64), 20, replace=False).tolist():
            c.put(r, x, 1 + int(c.rng.integers(0, 1000)))
    c.runs = [("num-kmers", 3, ()), ("num-kmers", 9, ()), ("num-kmers", 12, ()), ("jaccard", 9, ())]
    return c


# hub lines of the digit cases: rows and columns on both sides of a tile edge and in the partial last block of a 300 x 330 rectangle
DIGIT_NR, DIGIT_NC = 300, 330
HUB_ROWS, HUB_COLS = (0, 63, 64, 299), (0, 65, 127, 329)
DIGIT_VALUES = {
    "digit0": (4 ** np.arange(16), 5, 0),
    "digit1": (65536 * (1 + np.arange(100)), 40, 1),
    "digit2": (256 + np.arange(256), 100, 2),
    "digit3": ((1 << 23) + np.arange(256), 100, 3),
}
COLLAPSE_VALUES = (1 << 24) + 1 + 2 * np.arange(200)      # 200 cells on 101 float keys


def digit_case(name):
    """num-kmers with every count 1000: the proxy is the cell.  Every hub row holds `values` on columns that are no hubs, every hub column on
    rows that are no hubs; a thin fill touches the other tiles.  The pass that settles the cut is asserted on the host (test_the_cases_hold)."""
    if name == "collapse":
        values, count = COLLAPSE_VALUES, count_inside_key(key_of(COLLAPSE_VALUES), 50)
    else:
        values, count, _ = DIGIT_VALUES[name]
    c = Rect(name, DIGIT_NR, DIGIT_NC, 1000, 1000, [("num-kmers", count, ())])
    for r in HUB_ROWS:
        c.row_line(r, values, avoid=HUB_COLS)
    for x in HUB_COLS:
        c.col_line(x, values, avoid=HUB_ROWS)
    hub_r, hub_c = set(HUB_ROWS), set(HUB_COLS)
    for r, x, v in zip(c.rng.integers(0, c.nr, 400).tolist(), c.rng.integers(0, c.nc, 400).tolist(), c.rng.integers(1, 50, 400).tolist()):
        if r not in hub_r and x not in hub_c and (r, x) not in c.cells:
            c.put(r, x, v)
    return c


def line_values(case, row=None, col=None):
    r, c, v = case.triplets()
    return v[r == row] if row is not None else v[c == col]


def unrankable_case(side):
    """criterion min (and the measures on it): a sample of k-mer count 0 makes min(a, b) = 0 and the proxy of every cell beside it infinite.
    side "row": row sample 70 has count 0 — its line comes out whole, and so does the line of every column sample that holds one of its cells;
    side "col": the same with column sample 70.  The other lines hold 40 rankable cells and are cut."""
    nr, nc = 100, 140
    c = Rect("unrankable_" + side, nr, nc, 0, 0)
    c.a = 2000 + c.rng.integers(0, 500, nr)
    c.b = 3000 + c.rng.integers(0, 500, nc)
    if side == "row":
        c.a[70] = 0
        for x in (3, 64, 70, 139):
            c.put(70, x, 50 + x)
    else:
        c.b[70] = 0
        for r in (3, 63, 64, 99):
            c.put(r, 70, 50 + r)
    c.fill(0.4, 1, 1500)
    c.runs = [(cr, 2, ()) for cr in ("min", "ani-shorter", "cosine", "jaccard", "num-kmers")]
    return c


def unrankable_lines(case, criterion):
    """the slots (global ids) whose line holds a cell the device cannot rank"""
    r, c, v = case.triplets()
    bad = key_of(proxy_of(criterion, v, case.a[r], case.b[c])) == KEY_BEST
    return set((case.nc + r[bad]).tolist()) | set(c[bad].tolist())


def refetch_case():
    """num-kmers:3 under -min jaccard.  Row sample 10 (count 1000): its three largest cells are 600, 550 and X = 500, X beside column sample 200 of
    count 10 000 — jaccard 500 / 10 500, the smallest of the rectangle; the bound is one ulp above it, so X passes the widened bound, fails the
    exact one, and the line has two exact passes at or above its cut: it is fetched again, and the cell that takes X's place (400) lay below
    the cut.  Column sample 20 mirrors it with row sample 150 of count 10 000.  Every other cell has counts 1000 / 1000 and a value >= 100:
    jaccard >= 100 / 1900."""
    nr, nc = 160, 210
    c = Rect("refetch", nr, nc, 1000, 1000)
    c.a[150] = 10_000
    c.b[200] = 10_000
    c.put(10, 200, 500)
    c.put(150, 20, 500)
    for x, v in zip((5, 64, 130, 190, 66, 7), (600, 550, 400, 300, 200, 100)):
        c.put(10, x, v)
    for r, v in zip((5, 64, 130, 159, 66, 7), (600, 550, 400, 300, 200, 100)):
        c.put(r, 20, v)
    m = c.rng.random((nr, nc)) < 0.2
    for r, x in zip(*np.nonzero(m)):
        if r not in (10, 150) and x not in (20, 200) and (int(r), int(x)) not in c.cells:
            c.put(int(r), int(x), 100 + int(c.rng.integers(0, 300)))
    bound = float(np.nextafter(500.0 / 10_500.0, 2.0))
    c.runs = [("num-kmers", 3, (("jaccard", bound, None),))]
    return c


BIG = 65_600                                            # 65 600 x 65 600 cells = 17.2 GB: the offsets of the last rows exceed 2^32 cells


def big_case():
    """a zero rectangle with a handful of cells in its last two rows and last two columns"""
    c = Rect("big", BIG, BIG, 0, 0)
    c.a = 5000 + np.arange(BIG) % 977
    c.b = 7000 + np.arange(BIG) % 991
    for r, x, v in ((BIG - 1, BIG - 1, 900), (BIG - 1, 0, 800), (BIG - 1, 65_535, 700), (BIG - 1, 65_536, 650), (BIG - 2, BIG - 1, 600), (BIG - 2, 64, 500),
                    (0, BIG - 1, 400), (65_535, BIG - 2, 300), (65_536, BIG - 2, 250), (40_000, BIG - 1, 200), (BIG - 2, BIG - 2, 100), (BIG - 1, 33_000, 50)):
        c.put(r, x, v)
    c.runs = [("jaccard", 8, ()), ("jaccard", 2, ())]     # every line whole (the longest holds 5 cells); the longer lines cut
    return c


_CASES = {}


def case(name):
    if name not in _CASES:
        if name.startswith("shape_"):
            nr, nc = (int(x) for x in name[6:].split("x"))
            _CASES[name] = shape_case(nr, nc)
        elif name in DIGIT_VALUES or name == "collapse":
            _CASES[name] = digit_case(name)
        else:
            _CASES[name] = {"column_edge": column_edge, "unrankable_row": lambda: unrankable_case("row"), "unrankable_col": lambda: unrankable_case("col"),
                            "refetch": refetch_case, "big": big_case}[name]()
    return _CASES[name]


SHAPE_NAMES = ["shape_%dx%d" % s for s in SHAPES]
DIGIT_NAMES = list(DIGIT_VALUES) + ["collapse"]
