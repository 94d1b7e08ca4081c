"""Inputs and references of test_all2all_rows_records.py: a numpy restatement of the band window of the apply stage's write-back (which cells of
tile (X, Y) fall into the rows [row_lo, row_hi) and where they land in the band buffer), the brute force it is checked against, the bands the
tests take on a forest of block width `width`, and join_forest with two more block rows that no joined node reaches.

The forests themselves are variant_cases' (edge_forest, light_forest), wide_cases' (wide, join, stream) and all2all_rows_cases' (deep_forest)."""
import functools

import numpy as np

import all2all_rows_cases as RC
import variant_cases as VC
import wide_cases as W

tri = RC.tri
SENTINEL = 0xA5A5A5A5


# ------------------------------------------------------------------------------------------------------------------------------------
# the window
# ------------------------------------------------------------------------------------------------------------------------------------
def block_rows(width, lo, hi):
    """(Xlo, Xhi) of a non-empty band: the block rows it meets"""
    assert lo < hi
    return lo // width, (hi - 1) // width


def culled(width, lo, hi, X):
    xlo, xhi = block_rows(width, lo, hi)
    return X < xlo or X > xhi


def tile_window(width, N, lo, hi, X, Y):
    """What the write-back of tile (X, Y), X >= Y, does under the band [lo, hi): (r, c, offset) of every cell it may write — tile row r, tile column
    c, the word of the band buffer — as three arrays.  A cell is written iff lo <= row < hi on top of row < N and col < row; it lands at
    tri(row) - tri(lo) + col.  A culled tile writes nothing."""
    if culled(width, lo, hi, X):
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    r, c = np.meshgrid(np.arange(64, dtype=np.int64), np.arange(64, dtype=np.int64), indexing="ij")
    row, col = X * width + r, Y * width + c
    # (a tile is 64 x 64 accumulators whatever the width: rows and columns from `width` on belong to the next block and are never set by a mask)
    ok = (r < width) & (c < width) & (row < N) & (col < row) & (row >= lo) & (row < hi)
    off = row * (row - 1) // 2 - tri(lo) + col
    return r[ok], c[ok], off[ok]


def slice_tile_window(width, N, lo, hi, X):
    """The same for the diagonal tile (X, X) as the slice kernel addresses it: a base relative to the band's first cell — tri(rb) + rb - tri(lo), rb =
    X * width, which may be negative — plus a 32-bit lane offset rb * r + r (r - 1) / 2 + c; rows [first, lim) of the block are the band's."""
    if culled(width, lo, hi, X):
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    rb = X * width
    base = tri(rb) + rb - tri(lo)
    first = max(lo - rb, 0)
    lim = min(hi - rb, N - rb)
    r, c = np.meshgrid(np.arange(64, dtype=np.int64), np.arange(64, dtype=np.int64), indexing="ij")
    ok = (c < r) & (r >= first) & (r < lim) & (r < width)
    lane = rb * r + r * (r - 1) // 2 + c
    assert lane.max() < (1 << 32)
    return r[ok], c[ok], (base + lane)[ok]


def brute_window(width, N, lo, hi, X, Y):
    """cell by cell: the set {(r, c, offset)} of the cells of the triangle that lie in tile (X, Y) and in a row of the band"""
    out = set()
    for row in range(max(lo, X * width), min(hi, N, (X + 1) * width)):
        for col in range(Y * width, min(row, (Y + 1) * width)):
            out.add((row - X * width, col - Y * width, tri(row) + col - tri(lo)))
    return out


def window_bands(width, N):
    """bands that start and end on a block edge, one before it, one after it, and inside a single block"""
    w = width
    bands = [(w, 2 * w), (w - 1, 2 * w - 1), (w + 1, 2 * w + 1), (w - 1, 2 * w + 1), (w + 1, 2 * w - 1), (w + 3, w + 9), (w, w + 1), (2 * w - 1, 2 * w),
             (0, w), (0, 1), (1, 2), (0, N), (N - 1, N), (2 * w, N), (2 * w + 1, N)]
    return [(a, min(b, N)) for a, b in bands if a < min(b, N)]


# ------------------------------------------------------------------------------------------------------------------------------------
# the bands of the device tests
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_case(width, N):
    """(forest, definition) of variant_cases.edge_forest(width, N): computed once per process, shared, never written to"""
    pat = VC.edge_forest(width, N)
    exp = VC.definition(pat, N)
    exp.setflags(write=False)
    return pat, exp


def one_row_bands(width, N):
    """every one-row band from width - 1 to width + 1 and from 2 width - 1 to N"""
    rows = list(range(width - 1, width + 2)) + list(range(2 * width - 1, N))
    return [(r, r + 1) for r in rows]


def block_bands(width, N):
    """one block row, two, a row range inside one block, all of it"""
    w = width
    return [(w, 2 * w), (2 * w, min(4 * w, N)), (w + 3, w + 9), (0, N)]


def extended_join_forest(width=32):
    """wide_cases.join_forest (40 blocks, every one of them in some joined node's list) with two more block rows, 40 and 41, that hold narrow
    patterns only: a band over them lies outside every second-level tile with a list.  Returns (pat, N)."""
    base = W.join_forest(width)
    par = base["parent"].numpy()
    w = base["num_kmers"].numpy()
    lp, ids = base["local_ptr"].numpy(), base["local_ids"].numpy()
    F = VC._Forest()
    for p in range(1, len(par)):
        assert F.add(ids[lp[p]: lp[p + 1]], int(par[p]), int(w[p])) == p
    b40, b41 = 40 * width, 41 * width
    r = F.add([b40 + 1, b40 + 5, b40 + 31], -1, 3)
    F.add([b41 + 2], r, 200)
    F.add([b41, b41 + 7, b41 + 31], -1, 127)
    F.add([5, b40 + 9], -1, 128)                                 # a column in block 0: tile (40, 0)
    return F.pat(), 42 * width
