"""Inputs and references of test_all2all_rows_tiled.py: the band of the matrix restated the way the tiled call computes it (difference entries per
tile of columns, then a uint32 prefix sum), host censuses of its hits and jobs, and forests that hold the edges of a tile of 64 columns and of
the shares of a row's hits on purpose.  Forests are the dicts of all2all_rows_cases."""
import numpy as np

import all2all_rows_cases as RC
import variant_cases as VC

DEFAULT_TILE_COLS = 16384          # (the library's defaults: README, the table of switches)
DEFAULT_TILE_HITS = 256
MAX_TILE_COLS = 40896


def _subtree_weights(pat):
    """subtree weight of every node modulo 2^32 (a parent has a smaller index than its children)"""
    par = pat["parent"].numpy()
    W = pat["num_kmers"].numpy().astype(np.uint64)
    for p in range(len(par) - 1, 0, -1):
        if par[p] >= 0:
            W[par[p]] += W[p]
    return W & np.uint64(0xFFFFFFFF)


def hit_list(pat, lo, hi):
    """[(row, node)]: every local id inside [lo, hi) of a node that can add anything (local ids of its own, two ids or more in its full list, a
    subtree weight that is not 0 modulo 2^32) — the records of the hit passes"""
    W = _subtree_weights(pat)
    n, l = pat["num_samples"].numpy(), pat["num_local"].numpy()
    lp, ids = pat["local_ptr"].numpy(), pat["local_ids"].numpy()
    ok = (l > 0) & (n > 1) & (W != 0)
    node = np.repeat(np.arange(len(l)), l)
    m = ok[node] & (ids >= lo) & (ids < hi)
    return [(int(r), int(p)) for r, p in zip(ids[m], node[m])]


def hits(pat, lo, hi):
    return len(hit_list(pat, lo, hi))


def jobs(pat, lo, hi, tile_cols, tile_hits):
    """workgroups of the apply launch: for every row r > 0 with h hits, every tile of columns in front of r times every share of the hits"""
    per_row = np.bincount(np.array([r for r, _ in hit_list(pat, lo, hi)], dtype=np.int64), minlength=hi + 1)
    return int(sum(-(-r // tile_cols) * -(-int(per_row[r]) // tile_hits) for r in range(max(lo, 1), hi) if per_row[r]))


def _runs(ids):
    """an ascending id array as maximal runs of consecutive ids: [(start, len)]"""
    if ids.size == 0:
        return []
    cut = np.flatnonzero(np.diff(ids) != 1) + 1
    starts = np.concatenate(([0], cut))
    ends = np.concatenate((cut, [ids.size]))
    return [(int(ids[a]), int(b - a)) for a, b in zip(starts, ends)]


def band_by_runs(pat, N, lo, hi, tile_cols):
    """Rows [lo, hi) of all2all as the tiled call forms them.  For a hit (r, p) and a tile [c0, c0 + tile_cols) in front of r, every run [s, s + len)
    of p's full list, clipped to the tile and to ids < r, enters +W_p at its first column and -W_p (modulo 2^32) behind its last — left out on the
    tile's end and at r —; the inclusive uint32 prefix sum of the tile's entries is added to the band.  Returns (cells, runs, updates)."""
    W = _subtree_weights(pat)
    full = VC.full_lists(pat)
    exp = np.zeros(RC.tri(hi) - RC.tri(lo), dtype=np.uint32)
    n_runs = n_updates = 0
    for r, p in hit_list(pat, lo, hi):
        w = np.uint32(W[p])
        runs = _runs(full[p][full[p] < r])
        for c0 in range(0, r, tile_cols):
            cend = min(c0 + tile_cols, r)
            tile = np.zeros(tile_cols, dtype=np.uint64)                      # (entries modulo 2^32, kept in 64 bits: numpy warns when a uint32 wraps)
            for s, ln in runs:
                a, b = max(s, c0), min(s + ln, cend)
                if a < b:
                    tile[a - c0] = (int(tile[a - c0]) + int(w)) & 0xFFFFFFFF
                    if b < cend:
                        tile[b - c0] = (int(tile[b - c0]) - int(w)) & 0xFFFFFFFF
                    n_runs += 1
                    n_updates += b - a
            cells = (np.cumsum(tile, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)[: cend - c0]
            base = RC.tri(r) - RC.tri(lo) + c0
            exp[base: base + cend - c0] += cells
    return exp, n_runs, n_updates


# ------------------------------------------------------------------------------------------------------------------------------------
# forests: (pat, N)
# ------------------------------------------------------------------------------------------------------------------------------------
def tile_edge_forest():
    """N = 304, for tiles of 64 columns.  A root with the ids 0 .. 199: its runs cross columns 64 and 128, its rows 64 / 65 / 128 / 129 end in a
    tile of 64 columns or of one.  {40 .. 63, 70 .. 127, 300}: a run that ends at column 63 and one that ends at 127, the closing entry on the
    tile's end.  {64 .. 80, 301}: a run that starts at column 64; for row 301 the tiles [0, 64) and [128, 301) hold none of its ids.  A chain
    {0, 1} > {150 .. 160} > {302} and > {250, 303}: for row 302 the tile [192, 256) lies behind every ancestor's last id, for row 303 the tile
    [0, 64) lies in front of {250, 303}'s first possible id (161) — chain nodes skipped by their id range."""
    F = VC._Forest()
    F.add(range(200), -1, 3)
    F.add(list(range(40, 64)) + list(range(70, 128)) + [300], -1, 5)
    F.add(list(range(64, 81)) + [301], -1, 7)
    d = F.add([0, 1], -1, 2)
    e = F.add(range(150, 161), d, 11)
    F.add([302], e, 13)
    F.add([250, 303], e, (1 << 32) - 6)
    return F.pat(), 304


def five_hits_forest():
    """N = 70: five patterns hold sample 69 as a local id (row 69 has five hits), one of them under a parent; columns either side of 64"""
    F = VC._Forest()
    F.add([0, 1, 2, 69], -1, 1)
    F.add([10, 69], -1, 2)
    r = F.add([20, 21, 64, 65], -1, 4)
    F.add([66, 69], r, 8)
    F.add(list(range(30, 50)) + [69], -1, 16)
    F.add([63, 64, 69], -1, (1 << 32) - 3)
    return F.pat(), 70
