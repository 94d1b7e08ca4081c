"""Tables of tests/test_distance_pieces.py: one table of 258 rows for each source of cells that lies in HBM (the triangle, the rows of a batch of
queries, a CSR), and the cuts they are asked for in.  Host only.

258 rows: the launch that sizes the rows (a lane per row, workgroups of 256) has a full workgroup and a second one of two lanes, and a piece
can begin at row 256.  No table holds a sample without k-mers, and none holds a cell within the margins inside which the device hands a cell to
the host (margin_hits, decided on the CPU): host_cells == 0 is a property of the tables.  The witness of every comparison is DC.Rules."""
import ctypes

import numpy as np

import distance_cases as DC
import distance_parts_cases as PC
import distance_query_cases as QC

ROWS = 258
CUTS = [(0, 1), (1, 256), (5, 5), (256, 257), (257, 258)]    # an empty piece in between: no bytes, and a call
MEASURES = ("jaccard", "mash")                                # one of correctly rounded operations only, one with a log
K_TRI = 21
CSR_COLS, CSR_ROW0, CSR_LONG_ROW = 300, 42, 100
CSR_EMPTY_ROWS = (0, 255, 256, 257)


def triangle(seed=258):
    """258 samples, 33 153 cells: 1 .. min(a, b) with 30 % zeros; one empty name and one of 80 bytes"""
    rng = np.random.default_rng(seed)
    n = ROWS
    counts = DC.random_counts(rng, n)
    top = np.minimum(counts[:, None], counts[None, :])
    cells = np.tril(np.where(rng.random((n, n)) >= 0.3, rng.integers(1, top + 1), 0), -1).astype(np.int64)
    names = [b"s%d" % i for i in range(n)]
    names[3] = b""
    names[256] = b"a-name-of-eighty-bytes-" + b"x" * 57
    tri = np.concatenate([cells[i, :i] for i in range(n)]).astype(np.uint32)
    return {"n": n, "counts": counts, "cells": cells, "names": names, "text": DC.dense_body(names, counts, cells, triangle=True), "tri": tri, "cache": {}}


def rectangle(seed=2583):
    """258 queries by 3 samples (QC.table: query 2 all zeros, query 1 without a name, the last one with 80 bytes of it)"""
    return QC.table(ROWS, 3, seed)


def csr(seed=2584):
    """258 rows over 300 columns: rows 0, 255, 256 and 257 hold no entry, row 100 holds 257 (a workgroup of lanes and one), the others 0 to 8.
    One stored entry has the count 0: the text of the table does not hold it and no form writes it."""
    rng = np.random.default_rng(seed)
    lengths = [int(x) for x in rng.integers(0, 9, ROWS)]
    for r in CSR_EMPTY_ROWS:
        lengths[r] = 0
    lengths[CSR_LONG_ROW] = 257
    lengths[7] = 3
    t = PC.make(CSR_COLS, ROWS, CSR_ROW0, lengths, seed)
    val = t["val"].copy()
    val[int(t["ptr"][7]) + 1] = 0
    return PC.finish(CSR_COLS, ROWS, CSR_ROW0, t["counts"], t["ptr"], t["col"], val)


def csr_without_entries():
    """n_cells = 0: names and line ends only"""
    return PC.make(CSR_COLS, ROWS, CSR_ROW0, [0] * ROWS, 5)


def triangle_triples(t):
    return [(int(t["cells"][i, j]), int(t["counts"][i]), int(t["counts"][j])) for i in range(t["n"]) for j in range(i)]


def rectangle_triples(t):
    return [(int(t["cells"][q, j]), int(t["query_counts"][q]), int(t["counts"][j])) for q in range(t["nq"]) for j in range(t["n"])]


def csr_triples(t):
    return [(int(t["val"][e]), int(t["row_counts"][r]), int(t["counts"][t["col"][e]])) for r, e in PC.entries(t)]


def margin_hits(L, measure, k, triples):
    """The (count, a, b) whose value the device may leave to the host (dev_code of csrc/distance.hip): not finite or of 10^12 and more; below
    10^-9 without being an exact zero; t = |v| * 10^6 + 0.5 within 2^-20 of an integer — for a log / sqrt measure within t * 2^-44 where that is
    more.  The device's value of such a measure is a few ulp off the host's: both margins are doubled for them."""
    m = DC.METRICS.index(measure)
    exact = measure in QC.EXACT
    hit = []
    for c, a, b in triples:
        v = L.kmdbh_metric(m, ctypes.c_uint32(c), ctypes.c_uint32(a), ctypes.c_uint32(b), k)
        if v == 0:
            if not exact:
                hit.append((c, a, b))
            continue
        x = abs(v) * 1000000.0 + 0.5
        margin = 2.0 ** -20 if exact else 2 * max(2.0 ** -20, x * 2.0 ** -44)
        if not abs(v) < 1e12 or (not exact and abs(v) < 2e-9) or abs(x - round(x)) <= margin:
            hit.append((c, a, b))
    return hit
