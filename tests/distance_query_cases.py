"""Tables for new2all -distance (tests/test_distance_query_rows.py): nq x N rectangles of common k-mer counts with the queries' own counts and
names, the bounds of the sparse form, and the margins inside which the device hands a cell to the host (dev_code in csrc/distance.hip),
restated for a check on the CPU.  The witness of every comparison is distance_cases.Rules over distance_cases.dense_body of the same table."""
import ctypes

import numpy as np

import distance_cases as DC

K_LEN = 21
FORMS = {  # name -> (flags of the device handle, state the restated loop starts in)
    "dense": ({}, {}),
    "phylip": ({"phylip": True}, {"phylip": True}),
    "sparse": ({"sparse_out": True}, {"sparse_out": True}),
}
EXACT = ("jaccard", "min", "max", "num-kmers")       # measures of correctly rounded operations only


def table(nq, n, seed):
    """Sample counts of 3 to 6 million, query counts of 1 to 3 million (none equals a column's), cells of 1 .. min(a, b) with 30 % zeros.  From
    three queries on: query 2's row is all zeros, query 1 has no name and the last one a name of 80 bytes."""
    rng = np.random.default_rng(seed)
    counts = DC.random_counts(rng, n)
    query_counts = rng.integers(1_000_000, 3_000_000, nq).astype(np.int64)
    assert not set(query_counts.tolist()) & set(counts.tolist())
    cells = np.zeros((nq, n), np.int64)
    for q in range(nq):
        for j in range(n):
            cells[q, j] = rng.integers(1, min(query_counts[q], counts[j]) + 1) if rng.random() >= 0.3 else 0
    names = [b"q%d" % q for q in range(nq)]
    if nq >= 3:
        cells[2, :] = 0
        names[1] = b""
        names[-1] = b"a-query-of-eighty-bytes-" + b"x" * 56
        assert len(names[-1]) == 80
    return finish(names, counts, query_counts, cells)


def finish(names, counts, query_counts, cells):
    cells = np.asarray(cells, np.int64).reshape(len(names), len(counts))
    return {"nq": len(names), "n": len(counts), "names": names, "counts": np.asarray(counts, np.int64), "query_counts": np.asarray(query_counts, np.int64),
            "cells": cells, "text": DC.dense_body(names, query_counts, cells), "flat": np.ascontiguousarray(cells, np.uint32).reshape(-1), "cache": {}}


def zero_counts():
    """query 1 has no k-mers, samples 2 and 4 have none: 0 / 0 in jaccard, min and ani-shorter, c / 0 in mash-query"""
    rng = np.random.default_rng(6)
    counts = DC.random_counts(rng, 6)
    counts[2] = counts[4] = 0
    query_counts = np.array([1_500_000, 0, 2_500_000, 1_200_000], np.int64)
    cells = np.zeros((4, 6), np.int64)
    for q in range(4):
        for j in range(6):
            m = min(query_counts[q], counts[j])
            cells[q, j] = rng.integers(1, m + 1) if m else 0
    return finish([b"z%d" % q for q in range(4)], counts, query_counts, cells)


def rounding_boundary():
    """c = 1 over max(a, b) = 2 000 000: the value is 5e-7, and value * 10^6 + 0.5 is the integer 1 — the sixth decimal turns on it"""
    counts = [2_000_000, 1_500_000, 2_000_000]
    query_counts = [2_000_000, 1_000_000]
    cells = [[1, 1, 3], [1, 7, 1]]
    return finish([b"r0", b"r1"], counts, query_counts, cells)


def bounds_for(L, t, measure):
    """as test_distance_matrix.bounds_for: on the measure (the median of the values of query 0's row: about half the cells pass whichever way
    the measure runs), on another criterion, on the count"""
    m = DC.METRICS.index(measure)
    q = 0
    vals = sorted(L.kmdbh_metric(m, ctypes.c_uint32(int(c)), ctypes.c_uint32(int(t["query_counts"][q])), ctypes.c_uint32(int(t["counts"][j])), K_LEN)
                  for j, c in enumerate(t["cells"][q]) if c and t["counts"][j])
    other = "max" if measure != "max" else "min"
    b = [(measure, vals[len(vals) // 2], None), (other, 0.05, 0.95)] if vals else [(other, 0.05, 0.95)]
    if measure != "num-kmers":
        b.append(("num-kmers", 1000, 4_500_000))
    return b


def split_bounds(bounds):
    kmer = [b for b in bounds if b[0] == "num-kmers"]
    return ([b for b in bounds if b[0] != "num-kmers"], int(kmer[0][1]) if kmer and kmer[0][1] is not None else 0,
            int(kmer[0][2]) if kmer and kmer[0][2] is not None else DC.M32)


def witness(L, t, measure, form, bounds=(), rows=None):
    """what `distance -host` writes for the rows [rows[0], rows[1]) of the dense table of counts of t"""
    other, lo, hi = split_bounds(bounds)
    r = DC.Rules(L, measure, K_LEN, t["counts"], bounds=other, kmer_lo=lo, kmer_hi=hi, triangle=False, cache=t["cache"], **FORMS[form][1])
    if rows is None:
        return r.rows(t["text"])
    lines = t["text"].split(b"\n")[rows[0]:rows[1]]
    return r.rows(b"".join(ln + b"\n" for ln in lines), rows[0])


def host_margin_cells(L, t, measure):
    """The cells of t whose value the device may leave to the host (dev_code): not finite or of 10^12 and more; below 10^-9 without being an
    exact zero; t = |v| * 10^6 + 0.5 within 2^-20 of an integer — for a log / sqrt measure within t * 2^-44 where that is more.  The device's
    value of such a measure is a few ulp off the host's, which this check sees: both margins are doubled for them."""
    m = DC.METRICS.index(measure)
    exact = measure in EXACT
    hit = []
    for q in range(t["nq"]):
        for j in range(t["n"]):
            v = L.kmdbh_metric(m, ctypes.c_uint32(int(t["cells"][q, j])), ctypes.c_uint32(int(t["query_counts"][q])), ctypes.c_uint32(int(t["counts"][j])), K_LEN)
            if v == 0:
                if measure not in EXACT and t["cells"][q, j]:          # a zero the device does not take for settled
                    hit.append((q, j))
                continue
            a = abs(v)
            if not a < 1e12 or (not exact and a < 2e-9):
                hit.append((q, j))
                continue
            x = a * 1000000.0 + 0.5
            margin = 2.0 ** -20 if exact else 2 * max(2.0 ** -20, x * 2.0 ** -44)
            if abs(x - round(x)) <= margin:
                hit.append((q, j))
    return hit
