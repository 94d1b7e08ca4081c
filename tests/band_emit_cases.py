"""Inputs and references of test_all2all_band_emit.py: the closed form of a band's geometry in the block-record pipeline's streams (what
kmdbh_band_streams must return), the bands the geometry is held to, and far_forest — a hand-made collection of 100 000 samples, 3 125 blocks of
32 ids and 4.88 M block pairs, beyond the 2^22 the whole-matrix pipeline keys.

The other forests are variant_cases' (edge_forest, light_forest), wide_cases' (wide) and all2all_rows_cases' (chain, long list, weights, wide
codes); the band of the matrix from the definition is all2all_rows_cases.band_definition."""
import functools

import numpy as np

import all2all_rows_cases as RC
import variant_cases as VC

tri = RC.tri
SENTINEL = 0xA5A5A5A5
STREAM_LIMIT = 1 << 22


def tri32(x):
    """streams in front of block row x: block (X, Y), Y <= X, is stream tri32(X) + Y"""
    return x * (x + 1) // 2


def geometry(width, lo, hi):
    """the closed form: the band [lo, hi) owns the streams of the block rows lo // width .. (hi - 1) // width, keyed from the first of them on"""
    if lo == hi:
        return {"x_lo": 0, "x_hi": 0, "n_rows": 0, "fits": 1, "n_streams": 0, "stream_base": 0}
    xlo, xhi = lo // width, (hi - 1) // width
    n = tri32(xhi + 1) - tri32(xlo)
    return {"x_lo": xlo, "x_hi": xhi, "n_rows": xhi - xlo + 1, "fits": int(n + 1 < STREAM_LIMIT), "n_streams": n, "stream_base": tri32(xlo)}


GEOMETRY_N = (1, 2, 63, 64, 65, 4100, 92640, 92641, 300000)
GEOMETRY_WIDTHS = (32, 50, 64)


def geometry_bands(width, N):
    """one-row bands at block edges, block-aligned bands, bands that cross an edge, [0, N), empty bands"""
    w = width
    bands = {(0, N), (0, 0), (N, N), (N // 2, N // 2), (N - 1, N), (0, 1)}
    for e in {w, 2 * w, (N // w) * w, (N // w - 1) * w, (N // 2 // w) * w}:
        bands |= {(e - 1, e), (e, e + 1), (e, e + w), (e - w, e), (e - 1, e + 1), (e - 3, e + w + 5), (e, e)}
    return sorted((a, b) for a, b in bands if 0 <= a <= b <= N)


def fits_flip(width):
    """(N, lo, hi_fits, hi_beyond): bands [lo, hi) from row 0 on whose streams are one short of the limit, and at it.  tri32(X + 1) + 1 < 2^22
    holds up to X + 1 = 2895 block rows (tri32(2895) = 4 191 960) and fails from 2896 on (4 194 856)"""
    rows_ok = 2895
    assert tri32(rows_ok) + 1 < STREAM_LIMIT <= tri32(rows_ok + 1) + 1
    return (rows_ok + 2) * width, 0, rows_ok * width, rows_ok * width + 1


# ------------------------------------------------------------------------------------------------------------------------------------
# beyond 2^22 block pairs
# ------------------------------------------------------------------------------------------------------------------------------------
FAR_N, FAR_WIDTH = 100000, 32
# (the last one: four block rows at the top, 12 494 streams — more than the one-pass sort's LDS holds a cursor for)
FAR_BANDS = ((FAR_N - 70, FAR_N), (49990, 50060), (0, 40), (FAR_N - 1, FAR_N), (92640, 92641), (FAR_N - 100, FAR_N))
CS_MAX_KEYS = 2048


def expected_row_mode(n_streams, forced, width, packed=True):
    """the record path band emit takes for a band of n_streams streams: the many-streams path beyond CS_MAX_KEYS streams, KMDB_ROW_MODE (forced: None, 0,
    1) followed — but 0 only as far as the one-pass sort's LDS holds the band: 2048 records of 16 bytes staged with a 4-byte destination (and a 4-byte key
    word unless the records are packed: width <= 54), 12 bytes of cursors per stream, 1 088 bytes of scan scratch and the kernel's own 1 024, in 160 KB"""
    rows = n_streams > CS_MAX_KEYS if forced is None else bool(forced)
    pk = packed and width <= 54
    if not rows and 2048 * (16 + (4 if pk else 8)) + 12 * n_streams + 1088 + 1024 > 160 * 1024:
        rows = True
    return int(rows)


@functools.lru_cache(maxsize=None)
def far_forest():
    """N = 100 000 at width 32: 3 125 blocks, tri32(3125) = 4 884 375 block pairs.  Narrow patterns (one block, two blocks) at the bottom, in the
    middle (either side of the block edge 50 016) and at the top; wide ones of 3, 10, 11 and 40 blocks that span the whole id range and reach the
    last row; a chain under a wide root; the weights 1, 127, 128 and 2^32 - 1.  Rows 92 640 (the first row beyond the whole pipeline's limit at
    width 32), 49 990 .. 50 059, 0 .. 39 and the last 70 all get cells.  Returns (pat, N)."""
    N, w = FAR_N, FAR_WIDTH
    NB = (N + w - 1) // w
    assert NB == 3125 and tri32(NB) + 1 >= STREAM_LIMIT
    W = (1, 127, 128, (1 << 32) - 1)
    F = VC._Forest()
    k = 0
    for X in (0, 1, 1562, 1563, 2895, 3123, 3124):                   # narrow: one block (masks of 2 ids, of many, either side of the 32 | 32 split)
        b = X * w
        for ids in ([b, b + 1], [b + 3, b + 30, b + 31], list(range(b + 5, b + 20)), [b + 31, b + 0][::-1]):
            F.add(ids, -1, W[k % 4]); k += 1
        r = F.add([b + 2, b + 7], -1, W[k % 4]); k += 1              # two blocks: a parent in X, children in X + 1 (one id, two ids) where there is one
        if X + 1 < NB:
            F.add([b + w + 1], r, W[k % 4]); k += 1
            F.add([b + w + 4, b + w + 31], r, W[k % 4]); k += 1
        F.add([b + 30, b + w + 0] if X + 1 < NB else [b + 30, b + 31], -1, W[k % 4]); k += 1      # a local list over two blocks
    for ids in ([50015, 50016], [49990, 50059], [49999, 50016, 50017], [92639, 92640], [5, 92640], [92640, 99999]):   # pairs across the bands' edges
        F.add(ids, -1, W[k % 4]); k += 1
    # wide: c blocks spread over the whole id range, the last id in the last row's block; every other one reaches row N - 1
    for c in (3, 10, 11, 40):
        for rep in range(2):
            blocks = sorted({int(round(x)) for x in np.linspace(rep, NB - 1, c)})
            assert len(blocks) == c
            ids = []
            for j, X in enumerate(blocks):
                ids += [X * w + (j + rep) % w, X * w + (j + 7 * rep + 9) % w]
            ids = sorted(set(i for i in ids if i < N))
            if rep == 0:
                ids = sorted(set(ids + [N - 1]))
            F.add(ids, -1, W[k % 4]); k += 1
    # a wide root (blocks 0, 781, 1562) with a chain under it that climbs through the middle band and the top
    par = F.add([9, 781 * w + 3, 49991], -1, 127)
    for i, x in enumerate((49995, 50016, 50040, 50059, 70000, 92640, 99930, 99931, 99950, 99998, 99999)):
        par = F.add([x], par, W[i % 4])
    # narrow patterns in rows 0 .. 39 with columns in them, and under a wide parent's first block
    F.add([0, 1, 2, 39], -1, 128)
    F.add([38, 39, 40], -1, (1 << 32) - 1)
    return F.pat(), N
