"""`new2all -sample-rows <criterion>:<count>` in the library: every query's best database samples selected on the device — the row-segment select of
csrc/sample_rows.hip (kmdb_sampled_from_rows_device on the crafted rectangles of query_sampled_cases.py), the exact one-sided decision
(kmdbh_query_rows_select), the batch entries (kmdb_new2all_batch_sampled, kmdb_new2all_batch_seq_alphabet_sampled) on real queries, and the
node entries (kmdb_node_new2all_batch_sampled, kmdb_node_new2all_batch_seq_alphabet_sampled), and the front-end — one device and -gpus 2, text,
-from-minhash and -multisample-fasta queries — against the reference's recorded sparse tables cut by the same rule.
Expected values never come from the code under test: they are the numpy restatement of the rule (query_sampled_cases.expected_rows) over
kmdbh_metric, which test_host_cpu.py pins to the reference."""
import ctypes
import os

import numpy as np
import pytest

import query_sampled_cases as C
from conftest import ROOT
from test_new2all_sparse import JAC, vdev, virus  # noqa: F401  (fixtures)
from test_sample_rows_conformance import handle  # noqa: F401  (fixture)
from test_sample_rows_device import S, dev, rows_of  # noqa: F401  (S, dev: fixtures)

ENTRIES = ("kmdb_new2all_batch_sampled", "kmdb_new2all_batch_seq_alphabet_sampled", "kmdb_sampled_from_rows_device", "kmdbh_query_rows_select",
           "kmdb_new2all_sample_stats_get", "kmdb_node_new2all_batch_sampled", "kmdb_node_new2all_batch_seq_alphabet_sampled",
           "kmdb_node_new2all_sample_stats_get")


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_additive(K):
    """the eight entry points are exported and declared, the header announces them, the ABI version stays 8"""
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    for name in ENTRIES:
        assert name in K.capi.EXPORTS and name + "(" in header and hasattr(L, name), name
    assert "#define KMDB_HAS_NEW2ALL_SAMPLED 1" in header and "#define KMDB_ABI_VERSION 8" in header
    assert L.kmdb_abi_version() == 8 and K.capi.ABI_VERSION == 8
    for name in ("new2all_sampled", "new2all_seq_sampled", "sampled_from_rows_device", "new2all_sample_stats"):
        assert hasattr(K.DeviceDB, name), name
    for name in ("new2all_sampled", "new2all_seq_sampled", "new2all_sample_stats"):
        assert hasattr(K.NodeDB, name), name
    assert hasattr(K, "query_rows_select")


def test_argument_checks_come_before_any_device_work(K):
    """refused under the entry's name with handles that are never looked at: NULL handle / out / rows, count 0, an unknown criterion, missing
    sample_kmers or query_kmers, an unknown metric in a filter, more than 12 bounds, cell_lo > cell_hi, cell_hi > nq * n_cols, n_cols = 0 or >= 2^32"""
    L = K.lib()
    raw = K.capi._Sparse()
    out = ctypes.byref(raw)
    fake = ctypes.create_string_buffer(1 << 16)                  # stands for a handle: a call refused on its arguments never reads it
    h = ctypes.cast(fake, ctypes.c_void_p)
    cnt = np.ones(4, np.uint32)
    p = cnt.ctypes.data
    u64 = np.zeros(4, np.uint64)
    one = K.capi._filters([("jaccard", 0.5, None)])
    bad = K.capi._filters([("jaccard", 0.5, None)])
    bad[0].metric = 99
    many = K.capi._filters([("jaccard", 0.0, None)] * 13)
    JACC = K.capi.METRICS.index("jaccard")

    def refused(rc, entry, what):
        msg = L.kmdb_last_error().decode()
        assert rc != 0 and msg.startswith(entry + ":") and what in msg, (entry, what, msg)

    calls = {
        ENTRIES[0]: lambda hd, o, f, n, s, cr, ct: L.kmdb_new2all_batch_sampled(hd, None, None, 0, f, n, s, cr, ct, o, None),
        ENTRIES[1]: lambda hd, o, f, n, s, cr, ct: L.kmdb_new2all_batch_seq_alphabet_sampled(hd, None, None, 0, 1.0, 0.0, 0, f, n, s, cr, ct, o, u64.ctypes.data, None),
        ENTRIES[2]: lambda hd, o, f, n, s, cr, ct: L.kmdb_sampled_from_rows_device(hd, h, 2, 2, 0, 4, p, f, n, s, cr, ct, o, None),
        ENTRIES[5]: lambda hd, o, f, n, s, cr, ct: L.kmdb_node_new2all_batch_sampled(hd, None, None, 0, f, n, s, cr, ct, o, None),
        ENTRIES[6]: lambda hd, o, f, n, s, cr, ct: L.kmdb_node_new2all_batch_seq_alphabet_sampled(hd, None, None, 0, 1.0, 0.0, 0, f, n, s, cr, ct, o, u64.ctypes.data, None),
    }
    for name, call in calls.items():
        for hd, o in ((None, out), (h, None)):
            refused(call(hd, o, None, 0, p, JACC, 3), name, "null argument")
        for fs, n, sk, crit, count, what in ((None, 0, p, JACC, 0, "count must be at least 1"), (None, 0, p, 99, 3, "unknown criterion"),
                                             (None, 0, p, -1, 3, "unknown criterion"), (None, 0, None, JACC, 3, "sample_kmers is NULL"),
                                             (one, 1, None, JACC, 3, "sample_kmers is NULL"), (None, 1, p, JACC, 3, "null argument"),
                                             (bad, 1, p, JACC, 3, "unknown metric"), (many, 13, p, JACC, 3, "more than 12 bounds")):
            refused(call(h, out, fs, n, sk, crit, count), name, what)
    e = ENTRIES[2]
    rows = lambda nq, nc, lo, hi, qk=p, cells=h: L.kmdb_sampled_from_rows_device(h, cells, nq, nc, lo, hi, qk, None, 0, p, JACC, 3, out, None)  # noqa: E731
    refused(rows(2, 2, 0, 4, qk=None), e, "query_kmers is NULL")
    refused(rows(2, 2, 3, 1), e, "cell_lo > cell_hi")
    refused(rows(2, 2, 0, 5), e, "cell_hi beyond")
    refused(rows(2, 0, 0, 0), e, "n_cols")
    refused(rows(2, 1 << 32, 0, 4), e, "n_cols")
    refused(rows(2, 2, 0, 4, cells=None), e, "null rows")
    e = ENTRIES[3]
    sel = lambda crit, count, qk, sk, fs=None, n=0, o=out: L.kmdbh_query_rows_select(crit, count, 18, qk, 2, sk, fs, n, None, 0, o)  # noqa: E731
    refused(sel(JACC, 3, p, p, o=None), e, "null argument")
    refused(sel(JACC, 0, p, p), e, "count must be at least 1")
    refused(sel(99, 3, p, p), e, "unknown criterion")
    refused(sel(JACC, 3, p, None), e, "sample_kmers is NULL")
    refused(sel(JACC, 3, None, p), e, "query_kmers is NULL")
    refused(sel(JACC, 3, p, p, bad, 1), e, "unknown metric")
    refused(L.kmdb_new2all_sample_stats_get(None, None), ENTRIES[4], "null argument")
    refused(L.kmdb_new2all_sample_stats_get(h, None), ENTRIES[4], "null argument")
    refused(L.kmdb_node_new2all_sample_stats_get(None, None), ENTRIES[7], "null argument")
    refused(L.kmdb_node_new2all_sample_stats_get(h, None), ENTRIES[7], "null argument")


def whole_part(c, lo=0, hi=None, reverse=False):
    """the cells of a range as one candidate part of nq rows (ascending columns, or descending)"""
    q, s, v = c.triplets(lo, hi)
    ptr = np.zeros(c.nq + 1, np.uint64)
    ptr[1:] = np.cumsum(np.bincount(q, minlength=c.nq))
    if reverse:
        order = np.lexsort((-s, q))
        s, v = s[order], v[order]
    return ptr, s.astype(np.uint32), v.astype(np.uint32)


def test_host_select_is_the_restated_rule(K):
    """kmdbh_query_rows_select against the restatement: every criterion with a != b (mash-query and max tell them apart), ties across the cut
    resolved by id, a count larger than a row, an empty row, nq = 1, a bound ON a cell's value, and the refetch bound"""
    c = C.case("width_3x2049")
    for criterion, count, filters in c.runs:
        got = K.query_rows_select(criterion, count, C.K_LEN, c.a, c.b, [whole_part(c)], filters)
        assert rows_of(got) == C.expected_rows(K, c, criterion, count, filters), (criterion, count)
        assert got.measure is not None and got.n_rows == c.nq
    # the score is kmdbh_metric(criterion, c, a = the QUERY's count, b = the sample's)
    got = K.query_rows_select("mash-query", 5, C.K_LEN, c.a, c.b, [whole_part(c)])
    want = [K.metric("mash-query", v, int(c.a[q]), int(c.b[o]), C.K_LEN) for q, row in enumerate(rows_of(got)) for o, v in row]
    assert got.measure.tolist() == want
    swapped = C.Rows("swapped", c.nq, c.nc, 0, 0)
    swapped.dense, swapped.a, swapped.b = c.dense, np.resize(c.b, c.nq), np.resize(c.a, c.nc)
    assert want != [K.metric("mash-query", v, int(c.b[o]), int(c.a[q]), C.K_LEN) for q, row in enumerate(rows_of(got)) for o, v in row]
    for criterion in ("jaccard", "max"):                # (mash-query divides by a alone: within a row it ranks by the cell whatever a is)
        assert C.expected_rows(K, c, criterion, 5) != C.expected_rows(K, swapped, criterion, 5), criterion
    # ties across the cut: 1 500 cells of one value, the five smallest ids stay
    t = C.case("tied")
    got = rows_of(K.query_rows_select("num-kmers", 5, C.K_LEN, t.a, t.b, [whole_part(t)]))
    assert got == C.expected_rows(K, t, "num-kmers", 5) and [o for o, _ in got[1]] == np.flatnonzero(t.dense[1])[:5].tolist() and len(got[0]) == 3
    # an empty row, and nq = 1
    z = C.case("zero")
    assert rows_of(K.query_rows_select("jaccard", 4, C.K_LEN, z.a, z.b, [whole_part(z)]))[1] == []
    one = C.case("width_1x65")
    assert rows_of(K.query_rows_select("jaccard", 5, C.K_LEN, one.a, one.b, [whole_part(one)])) == C.expected_rows(K, one, "jaccard", 5)
    # a bound ON a cell's value keeps the cell, from either side
    q, s = 2, int(np.flatnonzero(c.dense[2])[7])
    x = K.metric("jaccard", int(c.dense[q, s]), int(c.a[q]), int(c.b[s]), C.K_LEN)
    for fl in ((("jaccard", x, None),), (("jaccard", None, x),)):
        got = rows_of(K.query_rows_select("num-kmers", c.nc, C.K_LEN, c.a, c.b, [whole_part(c)], fl))
        assert got == C.expected_rows(K, c, "num-kmers", c.nc, fl) and (s, int(c.dense[q, s])) in got[q]
    r = C.case("refetch")
    (criterion, count, filters), = r.runs
    assert rows_of(K.query_rows_select(criterion, count, C.K_LEN, r.a, r.b, [whole_part(r)], filters)) == C.expected_rows(K, r, criterion, count, filters)


def test_host_select_does_not_depend_on_parts_or_order(K):
    """a pair listed twice and in two parts counts once; parts in either order; candidates in descending columns"""
    c = C.case("width_3x2049")
    want = C.expected_rows(K, c, "jaccard", 5)
    a, b = whole_part(c, 0, 3000), whole_part(c, 2500, None, reverse=True)          # 500 cells listed by both
    cuts = list(zip(a[0][:-1].astype(int), a[0][1:].astype(int)))
    twice = (a[0] * np.uint64(2), np.concatenate([np.tile(a[1][x:y], 2) for x, y in cuts]), np.concatenate([np.tile(a[2][x:y], 2) for x, y in cuts]))
    for parts in ([a, b], [b, a], [twice, b], [b, a, a]):
        assert rows_of(K.query_rows_select("jaccard", 5, C.K_LEN, c.a, c.b, parts)) == want
    empty = K.query_rows_select("jaccard", 5, C.K_LEN, c.a, c.b, [])
    assert empty.n_rows == c.nq and empty.nnz == 0


def test_the_cases_hold_what_they_are_named_for(K):
    """the census of the crafted device cases, from the restated keys: every digit case settles its cut in the pass it is named for; the exact
    cases have no other key inside the margin band; the collapse case has its cut inside one float key; the refetch case leaves fewer than
    `count` exact passes at or above the cut; the unrankable case holds rows of both kinds"""
    for name in C.DIGIT_NAMES:
        c = C.case(name)
        count = c.runs[0][1]
        for q in range(c.nq):
            p = C.row_proxies(c, "num-kmers", q)
            keys = C.key_of(p)
            if name == "collapse":
                ks = np.sort(keys)[::-1]
                assert len(np.unique(p)) == 200 and len(np.unique(keys)) == 101 and ks[count - 1] == ks[count]
            else:
                assert C.settle_digit(keys, count) == C.DIGIT_VALUES[name][2], name
                assert C.band_is_empty(c, "num-kmers", count, q) == (name in C.EXACT), name
    r = C.case("refetch")
    (criterion, count, filters), = r.runs
    (_, bound, _), = filters
    j = K.metric("jaccard", 500, 1000, 10_000, C.K_LEN)
    assert j < bound == np.nextafter(j, 2.0) and bound * (1 - C.WIDEN) < j
    vals = np.sort(r.dense[1][r.dense[1] != 0])[::-1]
    assert vals[:4].tolist() == [600, 550, 500, 400] and C.band_is_empty(r, "num-kmers", 3, 1)
    assert [v for _, v in C.expected_rows(K, r, criterion, count, filters)[1]].count(500) == 0
    assert sorted(v for _, v in C.expected_rows(K, r, criterion, count, filters)[1]) == [400, 550, 600]
    for q in (0, 2):                                    # the other rows: count cells pass the exact bound above the cut, nothing to fetch again
        assert len(C.expected_rows(K, r, criterion, count, filters)[q]) == 3 and C.band_is_empty(r, "num-kmers", 3, q)
    u = C.case("unrankable")
    assert C.unrankable_rows(u, "min") >= {0, 3} and C.unrankable_rows(u, "jaccard") == {1} and C.unrankable_rows(u, "mash-query") == {3}
    assert not C.unrankable_rows(u, "num-kmers") and 2 not in C.unrankable_rows(u, "cosine")
    t = C.case("tied")
    assert np.count_nonzero(t.dense[1]) == 1500 and len(np.unique(C.key_of(C.row_proxies(t, "jaccard", 1)))) == 1


# ---- GPU: crafted rectangles ----------------------------------------------------------------------------------------------------------------
def upload(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m, np.uint32).view(np.int32).reshape(-1)).cuda()


def check_call(K, db, c, cells, criterion, count, filters=(), lo=0, hi=None):
    """the candidates of the range: all nq rows, no measures, ascending distinct ids with the rectangle's values; per row a superset of the exact
    best `count` of the range and a subset of its non-zero cells inside the widened bounds; decided by the host they give the restated rule.
    `cells` holds the whole rectangle: the call gets the address of cell `lo`.  Returns (rows as sets, the widened cells per row, the stats)."""
    hi = c.nq * c.nc if hi is None else hi
    cand = db.sampled_from_rows_device(cells.data_ptr() + 4 * lo, c.nq, c.nc, criterion, count, c.a, c.b, lo, hi, filters)
    st = db.new2all_sample_stats()
    what = (c.name, criterion, count, lo, hi)
    assert cand.measure is None and cand.n_rows == c.nq, what
    want = C.expected_rows(K, c, criterion, count, filters, lo, hi)
    wide = C.widened_rows(c, filters, lo, hi)
    lines = []
    for q in range(c.nq):
        ids, vals = cand.row(q)
        ids = ids.astype(np.int64)
        assert (np.diff(ids) > 0).all() and (not len(ids) or (ids[0] >= 0 and ids[-1] < c.nc)), what + (q,)
        assert c.dense[q, ids].tolist() == vals.tolist(), what + (q,)
        lines.append(set(ids.tolist()))
        assert {o for o, _ in want[q]} <= lines[q] <= wide[q], what + (q,)
    assert rows_of(K.query_rows_select(criterion, count, C.K_LEN, c.a, c.b, [cand], filters)) == want, what
    assert st["candidates"] == cand.nnz, what
    n_slots = (hi - 1) // c.nc + 1 - lo // c.nc if hi > lo else 0
    if n_slots:
        assert st["triangle_reads"] == 6 + 2 * (st["rows_refetched"] > 0), what
        assert st["d2h_bytes"] >= 8 * (n_slots + 1) + 8 * cand.nnz, what
    return lines, wide, st, cand


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.WIDTH_NAMES)
def test_widths(K, handle, name):
    """rows of one cell, of one line, of a line and a cell, of one segment less a cell, one segment, one segment and a cell, two segments and a
    cell; one row and three; counts 1, 5, the row's candidates exactly and more than the row; every criterion on 3 x 2049"""
    c = C.case(name)
    db = handle(2)
    cells = upload(c.dense)
    for criterion, count, filters in c.runs:
        lines, wide, st, _ = check_call(K, db, c, cells, criterion, count, filters)
        assert st["rows_refetched"] == 0
        if count >= max(len(w) for w in wide):
            assert lines == wide and st["rows_truncated"] == 0
        elif c.nc >= 63 and count <= 5:
            assert st["rows_truncated"] == c.nq and all(len(ln) < len(w) for ln, w in zip(lines, wide))


@pytest.mark.gpu
def test_flat_ranges(K, handle):
    """ranges that cut a row, end on a segment border and one cell past it, lie inside one segment, are empty; rows outside the range are empty; two
    consecutive ranges whose candidates together give the whole result"""
    c = C.case("width_3x4097")
    assert c.nc == C.RANGE_NC
    db = handle(2)
    cells = upload(c.dense)
    for lo, hi in C.RANGES:
        for criterion, count in (("jaccard", 5), ("jaccard", 3000)):
            lines, wide, st, cand = check_call(K, db, c, cells, criterion, count, (), lo, hi)
            for q in range(c.nq):
                if hi <= lo or q < lo // c.nc or q > (hi - 1) // c.nc:
                    assert not lines[q]
            if count == 3000:
                assert lines == wide
            if hi == lo:
                assert cand.nnz == 0 and st["triangle_reads"] == 0
    for criterion, count in (("jaccard", 5), ("mash-query", 40)):
        parts = [db.sampled_from_rows_device(cells.data_ptr() + 4 * lo, c.nq, c.nc, criterion, count, c.a, c.b, lo, hi)
                 for lo, hi in ((0, C.SPLIT), (C.SPLIT, 3 * c.nc))]
        for order in (parts, parts[::-1]):
            assert rows_of(K.query_rows_select(criterion, count, C.K_LEN, c.a, c.b, order)) == C.expected_rows(K, c, criterion, count)


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.DIGIT_NAMES)
def test_digits(K, handle, name):
    """a cut settled in each of the four passes, and keys that collapse to one float (every tied key is emitted): every row is cut; in the exact
    cases the device emits exactly `count` cells per row and fetches nothing again"""
    c = C.case(name)
    db = handle(2)
    (criterion, count, filters), = c.runs
    lines, wide, st, cand = check_call(K, db, c, upload(c.dense), criterion, count, filters)
    assert st["rows_truncated"] == c.nq and st["rows_refetched"] == 0
    for q in range(c.nq):
        assert count <= len(lines[q]) < len(wide[q]), (name, q)
    if name in C.EXACT:
        assert cand.nnz == st["candidates"] == count * c.nq
    if name == "collapse":
        p = C.row_proxies(c, criterion, 0)
        keys = C.key_of(p)
        T = np.sort(keys)[::-1][count - 1]
        assert len(lines[0]) >= int((keys >= T).sum()) > count


@pytest.mark.gpu
def test_unrankable_cells_zero_rows_and_zero_counts(K, handle):
    """a sample count of 0 beside a non-zero cell, c = a + b, a query count of 0: a row with a cell the device cannot rank comes out whole, the
    others are cut; a zero row is empty"""
    c = C.case("unrankable")
    db = handle(2)
    cells = upload(c.dense)
    for criterion, count, filters in c.runs:
        lines, wide, st, _ = check_call(K, db, c, cells, criterion, count, filters)
        whole = C.unrankable_rows(c, criterion)
        for q in range(c.nq):
            if q in whole:
                assert lines[q] == wide[q], (criterion, q)
            else:
                assert len(wide[q]) > 20 and len(lines[q]) < len(wide[q]), (criterion, q)
    z = C.case("zero")
    cells = upload(z.dense)
    for criterion, count, filters in z.runs:
        lines, wide, st, _ = check_call(K, db, z, cells, criterion, count, filters)
        assert not lines[1] and len(lines[0]) == len(lines[2]) == count and st["rows_truncated"] == 2


@pytest.mark.gpu
def test_a_row_of_tied_cells_comes_out_in_ascending_columns(K, handle):
    """1 500 cells of one key: all are candidates, in ascending columns (check_call) without a sort; the host keeps the five smallest ids"""
    c = C.case("tied")
    db = handle(2)
    cells = upload(c.dense)
    for criterion, count, filters in c.runs:
        lines, wide, st, cand = check_call(K, db, c, cells, criterion, count, filters)
        assert len(lines[1]) == 1500 and len(lines[0]) == 3 and st["rows_truncated"] == 0


@pytest.mark.gpu
def test_refetch(K, handle):
    """a bound inside the margin band leaves the truncated row 1 short of `count` exact passes: it is fetched again whole (2 more passes), the
    other rows are not, and the result is exact (the cell that completes the row lay below its cut)"""
    c = C.case("refetch")
    db = handle(2)
    (criterion, count, filters), = c.runs
    lines, wide, st, _ = check_call(K, db, c, upload(c.dense), criterion, count, filters)
    assert st["rows_refetched"] == 1 and st["triangle_reads"] == 8 and st["rows_truncated"] == 3
    assert lines[1] == wide[1] and len(lines[1]) == 7
    assert len(lines[0]) == len(lines[2]) == 3


@pytest.mark.gpu
def test_offsets_beyond_32_bits(K, handle):
    """the last three rows of a 70 000 x 70 001 rectangle as the flat range [(nq - 3) n_cols, nq n_cols): q * N + col in 64 bits; the result is that
    of the same three rows as a rectangle of their own, and the working arrays are those of 3 slots (what comes back: 4 row pointers, 8 bytes
    per candidate, one counter)"""
    c = C.case("big")
    db = handle(2)
    cells = upload(c.dense)
    nq, nc = C.BIG_NQ, C.BIG_NC
    lo = (nq - 3) * nc
    qk = np.zeros(nq, np.uint32)
    qk[-3:] = c.a
    for criterion, count, filters in c.runs:
        small = db.sampled_from_rows_device(cells.data_ptr(), 3, nc, criterion, count, c.a, c.b)
        cand = db.sampled_from_rows_device(cells.data_ptr(), nq, nc, criterion, count, qk, c.b, lo, nq * nc)
        st = db.new2all_sample_stats()
        assert cand.n_rows == nq and int(cand.row_ptr[nq - 3]) == 0 and cand.nnz == small.nnz
        assert (cand.row_ptr[nq - 3:].astype(np.int64) == small.row_ptr.astype(np.int64)).all()
        assert cand.col.tolist() == small.col.tolist() and cand.val.tolist() == small.val.tolist()
        assert st["d2h_bytes"] == 8 * 4 + 8 * cand.nnz + 8 and st["rows_refetched"] == 0
        tail = (cand.row_ptr[nq - 3:].astype(np.uint64), cand.col, cand.val)
        assert rows_of(K.query_rows_select(criterion, count, C.K_LEN, c.a, c.b, [tail])) == C.expected_rows(K, c, criterion, count)
        assert (cand.nnz == 36) == (count == 40)


# ---- GPU: real queries ------------------------------------------------------------------------------------------------------------------------
class _Dense:
    """rows of kmdb_new2all_batch as a case of the restatement"""

    def __init__(self, dense, a, b):
        self.dense, self.a, self.b = dense, a.astype(np.int64), b.astype(np.int64)
        self.nq, self.nc = dense.shape
        self._expected = {}
    triplets = C.Rows.triplets


@pytest.mark.gpu
def test_batch_entries_on_the_virus_queries(K, virus, vdev):
    """kmdb_new2all_batch_sampled and the text entry on virus part 2 against virus_k18_part1.db = the restatement applied to the rows of
    kmdb_new2all_batch (which are the reference's recorded rows), for jaccard, ani, mash-query and num-kmers, with and without a bound; the
    measures are the scores; every row of 100 cells is truncated"""
    v = virus
    dense = vdev.new2all(v.qs)
    assert np.array_equal(dense, v.dense)
    c = _Dense(dense, v.a, v.b)
    for filters in ((), tuple(JAC)):
        for criterion, count in (("jaccard", 10), ("ani", 3), ("mash-query", 10), ("num-kmers", 10), ("jaccard", 200)):
            want = C.expected_rows(K, c, criterion, count, filters, k=v.k)
            got = vdev.new2all_sampled(v.qs, criterion, count, v.b, filters)
            st = vdev.new2all_sample_stats()
            assert rows_of(got) == want, (criterion, count, filters)
            score = [K.metric(criterion, x, int(v.a[q]), int(v.b[o]), v.k) for q, row in enumerate(want) for o, x in row]
            assert got.measure.tolist() == score
            assert st["triangle_reads"] >= 6 and st["candidates"] >= got.nnz and st["select_ms"] > 0
            if not filters and count <= 10:
                assert st["rows_truncated"] == 65 and got.nnz == 65 * count and st["candidates"] < 6500
            txt, cnt = vdev.new2all_seq_sampled(v.texts, criterion, count, v.b, filters)
            assert rows_of(txt) == want and np.array_equal(cnt, v.a.astype(np.uint64)) and txt.measure.tolist() == score
    some = [len(r) for r in C.expected_rows(K, c, "jaccard", 10, tuple(JAC), k=v.k)]
    assert min(some) < 10 <= max(some)                  # the bound leaves some rows below `count`


@pytest.mark.gpu
def test_batch_entries_refuse_what_they_cannot_serve(K, virus, dev):
    """a handle without hashtables; a query-shard handle (as kmdb_new2all_batch_sparse_filtered refuses it)"""
    v = virus
    plain = K.DeviceDB(K.HostDB(v.path, skip_hashtables=True), device=dev)
    with pytest.raises(K.KmdbError, match="kmdb_new2all_batch_sampled: database was uploaded without hashtables"):
        plain.new2all_sampled(v.qs[:2], "jaccard", 3, v.b)
    plain.close()
    shard = K.DeviceDB(v.h, device=dev, query_shard=(0, 2))
    with pytest.raises(K.KmdbError, match="kmdb_new2all_batch_sampled: a query shard"):
        shard.new2all_sampled(v.qs[:2], "jaccard", 3, v.b)
    with pytest.raises(K.KmdbError, match="kmdb_new2all_batch_seq_alphabet_sampled: a query shard"):
        shard.new2all_seq_sampled(v.texts[:2], "jaccard", 3, v.b)
    shard.close()


# ---- the front-end ----------------------------------------------------------------------------------------------------------------------------
def _cli(*args, env=None, check=True):
    import subprocess
    exe = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=None if env is None else dict(os.environ, **env))
    assert not check or r.returncode == 0, r.stderr
    return r


def golden_sampled(K, golden_dir, criterion, count, bound=None, table="virus.k18.n2a.sparse.csv", k=18, n=100):
    """the file `new2all -sample-rows criterion:count [-min jaccard:bound]` must write, from the reference's unfiltered sparse table
    (tests/golden/virus.k18.n2a.sparse.csv): of every line the pairs that pass the bound, the `count` best by kmdbh_metric with the counts on
    the file's own lines (score descending, then sample id ascending), in ascending id.  Returns (bytes, pairs per row before the cut, rows with
    a score tie across the cut)."""
    lines = open(os.path.join(golden_dir, table), "rb").read().split(b"\n")
    counts = [int(x) for x in lines[1].split(b",")[2:] if x]
    assert lines[1].startswith(b"query-samples,total-kmers,") and len(counts) == n
    want, sizes, ties = lines[:2], [], 0
    for ln in lines[2:]:
        if not ln:
            want.append(ln)
            continue
        f = ln.split(b",")
        a = int(f[1])
        cells = []
        for cv in f[2:-1]:
            c, v = (int(x) for x in cv.split(b":"))
            if bound is None or K.metric("jaccard", v, a, counts[c - 1], k) >= bound:
                cells.append((-K.metric(criterion, v, a, counts[c - 1], k), c, cv))
        sizes.append(len(cells))
        cells.sort()
        ties += len(cells) > count and cells[count - 1][0] == cells[count][0]
        want.append(b",".join(f[:2] + [cv for _, _, cv in sorted(cells[:count], key=lambda x: x[1])] + [b""]))
    return b"\n".join(want), sizes, ties


def test_the_golden_expectation(K, golden_dir):
    """the top 10 by jaccard of the reference's table, computed once: all 65 rows hold 100 pairs, so every row is truncated; 63 of the 65 rows have a score
    tie across the cut under jaccard:10 (near-identical genomes), so the rule "ties towards the smaller sample id" decides what almost every row keeps"""
    want, sizes, ties = golden_sampled(K, golden_dir, "jaccard", 10)
    assert sizes == [100] * 65 and ties == 63
    rows = [ln for ln in want.split(b"\n")[2:] if ln]
    assert len(rows) == 65 and all(len(r.split(b",")) == 2 + 10 + 1 for r in rows)
    print("rows with a score tie across the cut: jaccard:10 %d, num-kmers:10 %d" % (ties, golden_sampled(K, golden_dir, "num-kmers", 10)[2]))
    _, sizes, _ = golden_sampled(K, golden_dir, "jaccard", 10, 0.99)
    assert min(sizes) < 10 < max(sizes)                 # -min jaccard:0.99 leaves some rows below `count`


def test_front_end_refusals(K, tmp_path):
    """refused by name before the database is read (the database named does not exist), no output file: -sample-rows without a criterion, with
    -distance, and a criterion that is no measure"""
    out = str(tmp_path / "out.csv")
    for opts, what in ((["-sample-rows", "10"], "the random strategy"), (["-sample-rows", "jaccard:10", "-distance", "jaccard"], "does not go with -distance"),
                       (["-sample-rows", "nonsense:10"], "Sampling parameters error - unknown measure: nonsense")):
        r = _cli("new2all", *opts, str(tmp_path / "no.db"), str(tmp_path / "no.list"), out, check=False)
        assert r.returncode != 0 and what in r.stderr and "Loading k-mer database" not in r.stderr, (opts, r.stderr)
        assert not os.path.exists(out), opts
    usage = _cli(check=False).stderr
    assert "new2all: -sample-rows <criterion>:<count>" in usage and "KMDB_N2A_HOST_SAMPLER=1" in usage


@pytest.mark.gpu
def test_front_end(K, golden_dir, dev, tmp_path):
    """`new2all -sample-rows` on the virus files = the expectation computed from the reference's table: jaccard:10, ani:3, with -sparse, with the
    host's extractor, with -min jaccard:0.99 (some rows fall below `count`); KMDB_N2A_HOST_SAMPLER=1 writes the same bytes; KMDB_VERBOSE tells
    which path ran"""
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    LINE = "[kmdb] new2all: sampled batch of"
    cwd = os.getcwd()
    os.chdir(golden_dir)          # list entries are ./test/virus/data/<name>
    try:
        for tag, crit, count, opt, bound in (("j10", "jaccard", 10, [], None), ("a3", "ani", 3, [], None), ("j10min", "jaccard", 10, ["-min", "jaccard:0.99"], 0.99),
                                             ("n10", "num-kmers", 10, [], None)):
            want = golden_sampled(K, golden_dir, crit, count, bound)[0]
            arms = [("dev", [], {"KMDB_VERBOSE": "1"}, True), ("hosts", [], {"KMDB_VERBOSE": "1", "KMDB_N2A_HOST_SAMPLER": "1"}, False)]
            if tag == "j10":
                arms += [("sparse", ["-sparse"], None, None), ("hostx", ["-host-extract"], None, None)]
            if tag in ("j10", "j10min"):
                arms += [("g2", ["-gpus", "2"], {"KMDB_VERBOSE": "1"}, True), ("g2hosts", ["-gpus", "2"], {"KMDB_N2A_HOST_SAMPLER": "1"}, None)]
            for name, extra, env, line in arms:
                out = t("%s.%s.csv" % (tag, name))
                r = _cli("new2all", *extra, *opt, "-sample-rows", "%s:%d" % (crit, count), g("virus_k18_part1.db"), g("virus.seqs.part2.list"), out, env=env)
                assert open(out, "rb").read() == want, (tag, name)
                if line is not None:
                    assert (LINE in r.stderr) == line, (name, r.stderr)
    finally:
        os.chdir(cwd)


@pytest.mark.gpu
def test_front_end_minhash_and_multisample_queries(K, golden_dir, dev, tmp_path):
    """the k-mer half of a batch (-from-minhash: the stored words of <sample>.minhash, written here with -f 1 so that the table is the reference's own)
    and the multisample query source (every record of synth.synth.fa a query, against synth_k21.db): the expectation from the reference's tables
    cut by the rule; one device, -gpus 2 and the host sampler write the same bytes"""
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    cwd = os.getcwd()
    os.chdir(golden_dir)
    try:
        _cli("minhash", "-k", "18", "-f", "1", g("virus.seqs.part2.list"))
        _cli("new2all", "-from-minhash", "-sparse", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("mh.sparse.csv"))
        assert open(t("mh.sparse.csv"), "rb").read() == open(g("virus.k18.n2a.sparse.csv"), "rb").read()
        want = golden_sampled(K, golden_dir, "jaccard", 10)[0]
        for name, extra, env in (("dev", [], None), ("g2", ["-gpus", "2"], None), ("hosts", [], {"KMDB_N2A_HOST_SAMPLER": "1"})):
            _cli("new2all", "-from-minhash", *extra, "-sample-rows", "jaccard:10", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("mh.%s.csv" % name), env=env)
            assert open(t("mh.%s.csv" % name), "rb").read() == want, name
    finally:
        os.chdir(cwd)
    lst = tmp_path / "synth.list"
    lst.write_text(g("synth.synth") + "\n")
    for crit, count in (("jaccard", 2), ("num-kmers", 1), ("mash-query", 3)):
        want, sizes, _ = golden_sampled(K, golden_dir, crit, count, table="synth.n2a-sparse", k=21, n=5)
        assert sizes == [4, 4, 4, 1, 4]
        for name, extra, env in (("dev", [], None), ("g2", ["-gpus", "2"], None), ("hosts", [], {"KMDB_N2A_HOST_SAMPLER": "1"})):
            out = t("synth.%s.%d.%s.csv" % (crit, count, name))
            _cli("new2all", "-multisample-fasta", *extra, "-sample-rows", "%s:%d" % (crit, count), g("synth_k21.db"), str(lst), out, env=env)
            assert open(out, "rb").read() == want, (crit, count, name)


@pytest.mark.gpu
def test_batch_entries_on_synth_k21(K, golden_dir, dev):
    """both batch entries on the five records of synth.synth.fa against synth_k21.db (k = 21, rows of 4, 4, 4, 1 and 4 cells, one empty column) = the
    restatement applied to the rows of kmdb_new2all_batch, with and without a bound"""
    h = K.HostDB(os.path.join(golden_dir, "synth_k21.db"))
    d = K.DeviceDB(h, device=dev, with_hashtables=True)
    raw = open(os.path.join(golden_dir, "synth.synth.fa")).read()
    texts = [r.split("\n", 1)[1].replace("\n", "") for r in raw.split(">") if r]
    qs = [K.sort_unique(K.extract_kmers(x, h.k, h.fraction)) for x in texts]
    a, b = np.array([q.size for q in qs], np.uint32), h.sample_kmers.astype(np.uint32)
    dense = d.new2all(qs)
    assert dense.shape == (5, 5) and [int(np.count_nonzero(r)) for r in dense] == [4, 4, 4, 1, 4]
    c = _Dense(dense, a, b)
    for filters in ((), (("num-kmers", 30.0, None),)):
        for criterion, count in (("jaccard", 2), ("ani", 1), ("mash-query", 3), ("num-kmers", 2), ("jaccard", 9)):
            want = C.expected_rows(K, c, criterion, count, filters, k=h.k)
            assert rows_of(d.new2all_sampled(qs, criterion, count, b, filters)) == want, (criterion, count, filters)
            txt, cnt = d.new2all_seq_sampled(texts, criterion, count, b, filters)
            assert rows_of(txt) == want and np.array_equal(cnt, a.astype(np.uint64)), (criterion, count, filters)
    d.close()


# ---- GPU: the node ------------------------------------------------------------------------------------------------------------------------------
def _node_check(K, v, shards, devices):
    """both node entries = the restatement on the reference's rows (what the one-device call gives: test_batch_entries_on_the_virus_queries), with and
    without a bound that leaves rows below `count`; the stats are sums over the devices"""
    c = _Dense(v.dense, v.a, v.b)
    nd = K.NodeDB(v.h, shards, devices, partition="prefix-tables")
    for filters in ((), tuple(JAC)):
        for criterion, count in (("jaccard", 10), ("mash-query", 3), ("num-kmers", 200)):
            want = C.expected_rows(K, c, criterion, count, filters, k=v.k)
            got = nd.new2all_sampled(v.qs, criterion, count, v.b, filters)
            st = nd.new2all_sample_stats()
            assert rows_of(got) == want, (shards, criterion, count, filters)
            score = [K.metric(criterion, x, int(v.a[q]), int(v.b[o]), v.k) for q, row in enumerate(want) for o, x in row]
            assert got.measure.tolist() == score
            assert st["candidates"] >= got.nnz and st["triangle_reads"] >= 6 and st["select_ms"] > 0 and st["d2h_bytes"] >= 8 * st["candidates"]
            if not filters and count == 10:
                assert st["candidates"] < 6500 and st["rows_truncated"] >= 65
            txt, cnt = nd.new2all_seq_sampled(v.texts, criterion, count, v.b, filters)
            assert rows_of(txt) == want and np.array_equal(cnt, v.a.astype(np.uint64)) and txt.measure.tolist() == score
    assert nd.new2all_sampled([], "jaccard", 3, v.b).n_rows == 0
    return nd


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [1, 2, 3, 5])
def test_node(K, virus, dev, shards):
    """query shards 1, 2, 3 and 5 over the devices the box has: every device selects on its chunk of the summed rows, the host decides once"""
    nd = _node_check(K, virus, shards, list(range(min(K.device_count(), shards))))
    assert nd.stats()["call_ms"] > 0
    nd.close()


@pytest.mark.gpu
def test_node_refusals(K, virus, dev):
    """a node of another partition is refused under the entry's name"""
    v = virus
    pre = K.NodeDB(v.h, 2, [dev], partition="prefix")
    with pytest.raises(K.KmdbError, match="kmdb_node_new2all_batch_sampled: the node was uploaded with partition prefix;"):
        pre.new2all_sampled(v.qs[:2], "jaccard", 3, v.b)
    with pytest.raises(K.KmdbError, match="kmdb_node_new2all_batch_seq_alphabet_sampled: the node was uploaded with partition prefix;"):
        pre.new2all_seq_sampled(v.texts[:2], "jaccard", 3, v.b)
    pre.close()


_RCCL_CHILD = """
import os, sys
sys.path.insert(0, os.path.join(%r, "tests"))
sys.path.insert(0, %r)
import conftest  # noqa: F401
from _kmerdb_loader import import_kmerdb_amd
from oracle import oracle as O
import test_new2all_sampled as T
import test_new2all_sparse as S
K = import_kmerdb_amd()
v = S.Virus(K, O, %r)
nd = T._node_check(K, v, 2, [0])
st = nd.stats()
assert st["collective_ms"] > 0 and st["rccl_version"] > 0, st
nd.close()
print("rccl child ok")
"""


@pytest.mark.gpu
def test_node_with_the_reduce_scatter_on_one_rank(K, golden_dir, dev):
    """KMDB_NODE_FORCE_RCCL=1 in a child process (the switch is read once per process): two shards on one device with the rows going through the
    reduce-scatter of a one-rank communicator, so the select reads the collective's output chunk"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _RCCL_CHILD % (ROOT, ROOT, golden_dir)], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, KMDB_NODE_FORCE_RCCL="1"))
    assert r.returncode == 0 and "rccl child ok" in r.stdout, r.stderr[-3000:]
