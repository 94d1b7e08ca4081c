"""Inputs and witnesses of test_distance_parts.py: CSRs over a block row of an all2all-parts grid, crafted entry by entry.  Host only.

The collection has N = 200 samples; the block row is its last part, the NR = 12 samples with the global ids 188 .. 199.  A table is the CSR
(row_ptr uint64[NR + 1], col uint32 global and ascending within a row, val uint32 > 0), the counts of the whole collection and the row samples'
own counts and names.  The witness is never the device: it is DC.Rules(..., sparse_out=True) of tests/distance_cases.py over the "name,count,
col:val,..." text of the same CSR (DC.sparse_body), which is what `all2all-parts` writes for those rows and `distance -sparse` reads.

The row lengths are the places where the source can go wrong: 0, 1, 63, 64 and 65 entries (a wave of 64 lanes), 130 (more than one wave inside
a workgroup of 256), every one of the 199 columns a row of the last sample can hold, and empty rows first, in the middle and last.  A row of 256
or 257 entries (a workgroup of 256 lanes) does not fit 200 columns: those two rows have a table of 300 columns of their own (wide_table)."""
import ctypes

import numpy as np

import distance_cases as DC

N, NR, ROW0, K_LEN = 200, 12, 188, 18
ROW_LENGTHS = [0, 1, 63, 64, 65, 0, 130, 7, 5, 2, 199, 0]
PREFIX_COLS = [8, 9, 98, 99, 198]                        # 0-based columns whose printed prefix is 9, 10, 99, 100, 199: its width changes
EXACT = ("jaccard", "min", "max", "num-kmers")


def names_of(n, first=0):
    return [b"sample_%d" % (first + i) for i in range(n)]


def make(n, nr, row0, lengths, seed, fixed=None):
    """a table: row r (global id row0 + r) holds lengths[r] entries on random columns, fixed[r] (a column list) where given"""
    rng = np.random.default_rng(seed)
    counts = DC.random_counts(rng, n)
    cols, vals, ptr = [], [], [0]
    for r, ln in enumerate(lengths):
        c = np.array(sorted(fixed[r]), np.int64) if fixed and r in fixed else np.sort(rng.choice(n, ln, replace=False))
        assert len(c) == ln
        cols.append(c)
        vals.append(rng.integers(1000, 2_900_000, ln))
        ptr.append(ptr[-1] + ln)
    return finish(n, nr, row0, counts, np.array(ptr, np.uint64), np.concatenate(cols).astype(np.uint32), np.concatenate(vals).astype(np.uint32))


def finish(n, nr, row0, counts, ptr, col, val, row_counts=None):
    counts = np.asarray(counts, np.int64)
    row_counts = counts[row0:row0 + nr].copy() if row_counts is None else np.asarray(row_counts, np.int64)
    t = dict(n=n, nr=nr, row0=row0, counts=counts, row_counts=row_counts, ptr=np.asarray(ptr, np.uint64), col=np.asarray(col, np.uint32),
             val=np.asarray(val, np.uint32), names=names_of(n), row_names=names_of(nr, row0), cache={})
    dense = np.zeros((nr, n), np.int64)
    for r in range(nr):
        lo, hi = int(t["ptr"][r]), int(t["ptr"][r + 1])
        assert np.all(np.diff(t["col"][lo:hi].astype(np.int64)) > 0)
        dense[r, t["col"][lo:hi]] = t["val"][lo:hi]
    t["dense"] = dense
    t["text"] = DC.sparse_body(t["row_names"], [int(c) for c in row_counts], dense)
    return t


def main_table():
    return make(N, NR, ROW0, ROW_LENGTHS, 4242, fixed={8: PREFIX_COLS, 10: [c for c in range(N) if c != 198]})


def wide_table():
    """rows of 256 and 257 entries, the edge of a workgroup, between a row of 1 and an empty one"""
    return make(300, 4, 296, [1, 256, 257, 0], 77)


def empty_table():
    """nnz = 0"""
    return make(N, NR, ROW0, [0] * NR, 5)


def zero_counts_table():
    """column sample 17 and row sample 190 (row 2) hold no k-mers: their cells divide by zero under min (NaN or infinite: the host's)"""
    t = make(N, NR, ROW0, [3, 0, 4, 6, 0, 2, 0, 0, 1, 0, 5, 0], 99, fixed={0: [5, 17, 60], 2: [1, 17, 100, 150], 10: [0, 17, 18, 64, 199]})
    counts = t["counts"].copy()
    counts[17] = 0
    counts[190] = 0
    return finish(N, NR, ROW0, counts, t["ptr"], t["col"], t["val"])


def truncated_counts_table():
    """counts above 2^32: the text path keeps their low 32 bits, for the columns and for the row samples alike"""
    t = make(N, NR, ROW0, [4, 0, 9, 64, 0, 3, 0, 0, 2, 0, 40, 1], 123)
    counts = t["counts"].copy()
    counts[::7] += 1 << 32
    counts[189] += 5 << 32
    counts[198] += 1 << 33
    return finish(N, NR, ROW0, counts, t["ptr"], t["col"], t["val"])


def rounding_table():
    """max with a = b = 2 000 000 and a count of 1: the value 5e-7, t = v * 10^6 + 0.5 = 1 exactly: "0.000001" by the host's arithmetic"""
    counts = np.full(N, 2_000_000, np.int64)
    ptr = np.zeros(NR + 1, np.uint64)
    ptr[4:] = 2
    return finish(N, NR, ROW0, counts, ptr, [7, 100], [1, 3])


def value(L, t, measure, r, e):
    return L.kmdbh_metric(DC.METRICS.index(measure), ctypes.c_uint32(int(t["val"][e])), ctypes.c_uint32(int(t["row_counts"][r]) & DC.M32),
                          ctypes.c_uint32(int(t["counts"][t["col"][e]]) & DC.M32), K_LEN)


def entries(t):
    for r in range(t["nr"]):
        for e in range(int(t["ptr"][r]), int(t["ptr"][r + 1])):
            yield r, e


def bounds_for(L, t, measure):
    """A lower bound ON a cell's value — the median of the longest row's values: the device sees a bound within 10^-9 of its value and leaves the
    cell to the host, which keeps it (>=) — a pair on another criterion, and a bound on the count."""
    r = int(np.argmax(np.diff(t["ptr"].astype(np.int64))))
    vals = sorted(value(L, t, measure, r, e) for e in range(int(t["ptr"][r]), int(t["ptr"][r + 1])))
    other = "max" if measure != "max" else "min"
    b = [(measure, vals[len(vals) // 2], None), (other, 0.0005, 0.9)]
    if measure != "num-kmers":
        b.append(("num-kmers", 5000, 2_800_000))
    return b


def split_bounds(bounds):
    kmer = [b for b in bounds if b[0] == "num-kmers"]
    return ([b for b in bounds if b[0] != "num-kmers"], int(kmer[0][1]) if kmer and kmer[0][1] is not None else 0,
            int(kmer[0][2]) if kmer and kmer[0][2] is not None else DC.M32)


def witness(L, t, measure, bounds=(), rows=None):
    """what `distance -sparse` writes for the rows [rows[0], rows[1]) of the sparse table of counts of t"""
    other, lo, hi = split_bounds(bounds)
    r = DC.Rules(L, measure, K_LEN, t["counts"], bounds=other, kmer_lo=lo, kmer_hi=hi, sparse_out=True, triangle=False, cache=t["cache"])
    if rows is None:
        return r.rows(t["text"])
    lines = t["text"].split(b"\n")[rows[0]:rows[1]]
    return r.rows(b"".join(ln + b"\n" for ln in lines), rows[0])


def host_margin_entries(L, t, measure):
    """The entries of t whose value the device may leave to the host (dev_code of csrc/distance.hip): not finite or of 10^12 and more; below
    10^-9 without being an exact zero; t = |v| * 10^6 + 0.5 within 2^-20 of an integer — for a log / sqrt measure within t * 2^-44 where that is
    more.  The device's value of such a measure is a few ulp off the host's, which this check sees: both margins are doubled for them."""
    exact = measure in EXACT
    hit = []
    for r, e in entries(t):
        v = value(L, t, measure, r, e)
        if v == 0:
            if not exact:
                hit.append(e)
            continue
        a = abs(v)
        if not a < 1e12 or (not exact and a < 2e-9):
            hit.append(e)
            continue
        x = a * 1000000.0 + 0.5
        margin = 2.0 ** -20 if exact else 2 * max(2.0 ** -20, x * 2.0 ** -44)
        if abs(x - round(x)) <= margin:
            hit.append(e)
    return hit


# ---- the gather: the cells of a block row ------------------------------------------------------------------------------------------------------
GATHER_WIDTHS = [64, 1, 70, 53]                          # four earlier parts; with the diagonal's 12 samples the collection's 200
GATHER_EMPTY_CELL, GATHER_EMPTY_ROW = 1, 6


def gather_cells(seed=31):
    """-> [(row_ptr, col local to the cell, val, n_cols, col_shift)] for the four off-diagonal cells and the diagonal (lower triangle: row r holds
    columns < r).  The cell of width 1 is empty; row 6 is empty in every cell; row 3 of the first cell holds all 64 columns."""
    rng = np.random.default_rng(seed)
    cells, shift = [], 0
    for ci, w in enumerate(GATHER_WIDTHS + [NR]):
        diagonal = ci == len(GATHER_WIDTHS)
        ptr, col, val = [0], [], []
        for r in range(NR):
            room = r if diagonal else w
            ln = 0 if (ci == GATHER_EMPTY_CELL or r == GATHER_EMPTY_ROW) else (room if (ci == 0 and r == 3) else int(rng.integers(0, room + 1)))
            c = np.sort(rng.choice(room, ln, replace=False)) if ln else np.zeros(0, np.int64)
            col.append(c)
            val.append(rng.integers(1000, 2_900_000, ln))
            ptr.append(ptr[-1] + ln)
        cells.append((np.array(ptr, np.uint64), np.concatenate(col).astype(np.uint32), np.concatenate(val).astype(np.uint32), w, shift))
        shift += w
    assert shift == N
    return cells


def gathered(cells):
    """the concatenation, in numpy: row r = its entries of cell 0, cell 1, ..., the columns shifted"""
    ptr, col, val = [0], [], []
    for r in range(NR):
        for p, c, v, w, shift in cells:
            lo, hi = int(p[r]), int(p[r + 1])
            col.append(c[lo:hi].astype(np.int64) + shift)
            val.append(v[lo:hi].astype(np.int64))
        ptr.append(ptr[-1] + sum(int(p[r + 1] - p[r]) for p, _, _, _, _ in cells))
    return np.array(ptr, np.uint64), np.concatenate(col).astype(np.uint32), np.concatenate(val).astype(np.uint32)


def parse_rows(text):
    """the (column, text of the value) pairs of every row of a sparse measure table"""
    rows = []
    for ln in text.split(b"\n")[:-1]:
        f = ln.split(b",")
        assert f[-1] == b""
        rows.append((f[0], [(int(x.split(b":")[0]) - 1, x.split(b":")[1]) for x in f[1:-1]]))
    return rows
