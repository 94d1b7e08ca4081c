"""all2all-parts -distance: the table of a measure straight from the CSR of a block row of the grid in HBM (kmdb_distance_parts_begin_rows,
kmdb_distance_parts_add_db2db, kmdb_distance_parts_add_all2all, kmdb_distance_parts_add_csr_device, kmdb_distance_take_csr_device,
kmdb_distance_csr_rows, kmdb_distance_csr_device, kmdb_distance_csr_row_ptr, kmdb_distance_parts_stats_get; the front-end's
`all2all-parts -distance <measure>`).  The definition: byte for byte the file `all2all-parts L T` followed by `distance -sparse <measure> T out`
writes.  The witness is never the code under test: the row rules restated in tests/distance_cases.py over the sparse text of the same CSR
(tests/distance_parts_cases.py), the host loop run on the reference's recorded table, and the entries that are pinned by tests of their own
(kmdb_db2db_sparse_filtered, kmdb_all2all_sparse, all2all-sp -distance)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distance_cases as DC
import distance_parts_cases as PC
from conftest import ROOT
from test_parts_sampled import grid3  # noqa: F401  (fixture)
from test_sample_rows_device import S, dev  # noqa: F401  (fixtures of grid3)

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
ENTRIES = ("kmdb_distance_parts_begin_rows", "kmdb_distance_parts_add_db2db", "kmdb_distance_parts_add_all2all", "kmdb_distance_parts_add_csr_device",
           "kmdb_distance_take_csr_device", "kmdb_distance_csr_rows", "kmdb_distance_csr_device", "kmdb_distance_csr_row_ptr", "kmdb_distance_parts_stats_get")


@pytest.fixture(scope="module")
def L(K):
    lib = K.capi.lib()
    lib.kmdbh_metric.restype = ctypes.c_double
    return lib


@pytest.fixture(scope="module")
def main_table():
    return PC.main_table()


# ---- no device -------------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_parts_entry_points(K):
    hdr = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    assert re.search(r"^#define KMDB_HAS_DISTANCE_PARTS 1$", hdr, re.M) and "#define KMDB_ABI_VERSION 8" in hdr and K.ABI_VERSION == 8
    lib = K.capi.lib()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in K.capi.EXPORTS and name + "(" in hdr, name
    for method in ("parts_begin", "parts_add_db2db", "parts_add_all2all", "take_csr", "csr_rows", "csr_ptrs", "parts_stats"):
        assert hasattr(K.Distance, method), method


def test_null_arguments_are_refused_by_name(K):
    lib = K.capi.lib()
    calls = {
        "kmdb_distance_parts_begin_rows": lambda: lib.kmdb_distance_parts_begin_rows(None, 0, None, None),
        "kmdb_distance_parts_add_db2db": lambda: lib.kmdb_distance_parts_add_db2db(None, None, None, 0, None),
        "kmdb_distance_parts_add_all2all": lambda: lib.kmdb_distance_parts_add_all2all(None, None, 0, None),
        "kmdb_distance_parts_add_csr_device": lambda: lib.kmdb_distance_parts_add_csr_device(None, None, None, None, 0, 0),
        "kmdb_distance_take_csr_device": lambda: lib.kmdb_distance_take_csr_device(None, None, None, None, 0, None, None),
        "kmdb_distance_csr_rows": lambda: lib.kmdb_distance_csr_rows(None, 0, 0, None),
        "kmdb_distance_csr_device": lambda: lib.kmdb_distance_csr_device(None, None, None, None, None),
        "kmdb_distance_csr_row_ptr": lambda: lib.kmdb_distance_csr_row_ptr(None, None),
        "kmdb_distance_parts_stats_get": lambda: lib.kmdb_distance_parts_stats_get(None, None),
    }
    assert sorted(calls) == sorted(ENTRIES)
    for name, call in calls.items():
        assert call() != 0 and name.encode() + b":" in lib.kmdb_last_error(), name


def cli(argv, env_extra=None, cwd=None):
    return subprocess.run([EXE] + [str(a) for a in argv], capture_output=True, text=True, env=dict(os.environ, **(env_extra or {})), cwd=cwd)


def test_front_end_refusals(tmp_path):
    lst, out = tmp_path / "no-such.list", tmp_path / "out"
    r = cli(["all2all-parts", "-distance", "nosuch", lst, out])     # before any database is read: the list does not exist
    assert r.returncode != 0 and "unknown measure: nosuch" in r.stderr and "no-such" not in r.stderr
    r = cli(["all2all-parts", "-sample-rows", "jaccard:5", "-distance", "jaccard", lst, out])
    assert r.returncode != 0 and "-distance" in r.stderr and "-sample-rows" in r.stderr and "no-such" not in r.stderr
    r = cli(["all2all-parts", "-phylip-out", "-distance", "jaccard", lst, out])
    assert r.returncode != 0 and "-distance" in r.stderr and "-phylip-out" in r.stderr and "phylip output from sparse input" in r.stderr and "no-such" not in r.stderr
    r = cli(["all2all-parts", "-distance", "jaccard", lst, out])    # and a well-formed command line reaches the list
    assert r.returncode != 0 and "no-such.list" in r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".jaccard")
    assert "all2all-parts [-min ...]* [-max ...]* [-gpus <W>] -distance <measure> [-distance <measure>]* <db_list> <output>" in cli([]).stderr


def test_the_tables_hold_what_they_are_named_for(L, main_table):
    t = main_table
    lengths = np.diff(t["ptr"].astype(np.int64)).tolist()
    assert lengths == PC.ROW_LENGTHS and {0, 1, 63, 64, 65, 199} <= set(lengths) and lengths[0] == lengths[5] == lengths[-1] == 0
    assert t["col"][int(t["ptr"][8]):int(t["ptr"][9])].tolist() == PC.PREFIX_COLS
    assert np.diff(PC.wide_table()["ptr"].astype(np.int64)).tolist() == [1, 256, 257, 0]
    assert PC.empty_table()["ptr"][-1] == 0 and PC.empty_table()["text"].count(b"\n") == PC.NR
    # the table of the host-cell cap holds no entry within the host margins: decided on the CPU, with kmdbh_metric
    for measure in DC.METRICS:
        assert PC.host_margin_entries(L, t, measure) == [], measure
    # the bound of bounds_for lies ON an entry's value
    for measure in DC.METRICS:
        lo = PC.bounds_for(L, t, measure)[0][1]
        assert any(PC.value(L, t, measure, r, e) == lo for r, e in PC.entries(t)), measure
    z = PC.zero_counts_table()
    assert z["counts"][17] == 0 and z["row_counts"][2] == 0
    nan_or_inf = [PC.value(L, z, "min", r, e) for r, e in PC.entries(z) if z["col"][e] == 17 or r == 2]
    assert len(nan_or_inf) == 6 and all(not abs(v) < 1e12 for v in nan_or_inf)
    tr = PC.truncated_counts_table()
    assert (tr["counts"] >> 32).any() and (tr["row_counts"] >> 32).any()
    ro = PC.rounding_table()
    assert PC.witness(L, ro, "max") == b"".join(b"sample_%d,\n" % (PC.ROW0 + r) if r != 3 else b"sample_191,8:0.000001,101:0.000002,\n" for r in range(PC.NR))
    cells = PC.gather_cells()
    assert [c[3] for c in cells] == [64, 1, 70, 53, 12] and cells[PC.GATHER_EMPTY_CELL][0][-1] == 0
    assert all(c[0][PC.GATHER_EMPTY_ROW] == c[0][PC.GATHER_EMPTY_ROW + 1] for c in cells) and cells[0][0][4] - cells[0][0][3] == 64


# ---- the library, CSRs as torch tensors --------------------------------------------------------------------------------------------------------
class Dev:
    """a table's CSR in HBM"""

    def __init__(self, ptr, col, val):
        import torch
        self.ptr = torch.from_numpy(np.ascontiguousarray(ptr, np.uint64).view(np.int64)).cuda()
        self.col = torch.from_numpy(np.ascontiguousarray(col, np.uint32).view(np.int32)).cuda() if len(col) else None
        self.val = torch.from_numpy(np.ascontiguousarray(val, np.uint32).view(np.int32)).cuda() if len(val) else None

    def ptrs(self):
        return self.ptr.data_ptr(), self.col.data_ptr() if self.col is not None else None, self.val.data_ptr() if self.val is not None else None


def handle(K, t, measure, bounds=()):
    return K.Distance(measure, PC.K_LEN, t["counts"] & DC.M32, filters=bounds, sparse_out=True)


def taken(K, t, measure, bounds=()):
    dev_csr = Dev(t["ptr"], t["col"], t["val"])
    d = handle(K, t, measure, bounds)
    d.take_csr(*dev_csr.ptrs(), t["nr"], t["row_counts"], t["row_names"])
    return d, dev_csr


@pytest.mark.gpu
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounds"])
@pytest.mark.parametrize("measure", DC.METRICS)
def test_every_measure_from_the_csr(K, L, main_table, measure, bounded):
    t = main_table
    bounds = PC.bounds_for(L, t, measure) if bounded else []
    want = PC.witness(L, t, measure, bounds)
    d, keep = taken(K, t, measure, bounds)
    assert d.csr_rows(0, PC.NR) == want
    one_by_one = [d.csr_rows(r, r + 1) for r in range(PC.NR)]
    assert b"".join(one_by_one) == want and d.csr_rows(PC.NR, PC.NR) == b"" and d.csr_rows(3, 3) == b""
    assert one_by_one[4] == PC.witness(L, t, measure, bounds, rows=(4, 5))
    assert d.csr_rows(2, 7) == PC.witness(L, t, measure, bounds, rows=(2, 7))
    st = d.stats()
    nnz = int(t["ptr"][-1])
    assert st["calls"] == PC.NR + 4 and st["cells_read"] == 2 * nnz + int(t["ptr"][7] - t["ptr"][2]) and st["parse_ms"] == 0, st
    if bounded:
        # the bound on an entry's value: the host's (a bound on the count is an integer, which the device settles); about half the entries go
        assert (st["host_cells"] >= 1 or measure == "num-kmers") and want.count(b":") < nnz
    assert d.csr_row_ptr().tolist() == t["ptr"].tolist()
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("measure", DC.METRICS)
def test_the_host_cannot_carry_the_table(K, L, main_table, measure):
    t = main_table
    d, keep = taken(K, t, measure)
    assert d.csr_rows(0, PC.NR) == PC.witness(L, t, measure)
    st, nnz = d.stats(), int(t["ptr"][-1])
    assert st["cells_written"] == nnz and st["host_cells"] * 100 <= st["cells_written"], st
    d.close()


@pytest.mark.gpu
def test_rows_at_the_edge_of_a_workgroup_and_no_entries_at_all(K, L):
    for t in (PC.wide_table(), PC.empty_table()):
        for measure in ("jaccard", "cosine", "mash-query"):
            d, keep = taken(K, t, measure)
            assert d.csr_rows(0, t["nr"]) == PC.witness(L, t, measure), measure
            assert b"".join(d.csr_rows(r, r + 1) for r in range(t["nr"])) == PC.witness(L, t, measure), measure
            d.close()
    t = PC.empty_table()
    d = handle(K, t, "jaccard")
    d.take_csr(Dev(t["ptr"], [], []).ptr.data_ptr(), None, None, t["nr"], t["row_counts"], t["row_names"])    # no entries behind the null pointers
    assert d.csr_rows(0, t["nr"]) == PC.witness(L, t, "jaccard")
    d.close()


@pytest.mark.gpu
def test_counts_of_zero_are_the_hosts(K, L):
    t = PC.zero_counts_table()
    for measure in ("jaccard", "min", "mash-query", "ani-shorter"):
        d, keep = taken(K, t, measure)
        assert d.csr_rows(0, PC.NR) == PC.witness(L, t, measure), measure
        if measure in ("min", "ani-shorter"):
            assert d.stats()["host_cells"] >= 6, measure
        d.close()


@pytest.mark.gpu
def test_counts_above_32_bits_are_truncated_as_the_text_path_truncates_them(K, L):
    t = PC.truncated_counts_table()
    for measure in ("jaccard", "max", "mash-query"):
        d, keep = taken(K, t, measure)
        assert d.csr_rows(0, PC.NR) == PC.witness(L, t, measure), measure
        d.close()


@pytest.mark.gpu
def test_a_cell_on_the_rounding_boundary_is_the_hosts(K, L):
    t = PC.rounding_table()
    d, keep = taken(K, t, "max")
    got = d.csr_rows(0, PC.NR)
    assert got == PC.witness(L, t, "max") and b"sample_191,8:0.000001,101:0.000002,\n" in got
    assert d.stats()["host_cells"] == 2
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("measure", ["jaccard", "mash"])
def test_the_text_path_gives_the_same_bytes(K, L, main_table, measure):
    t = main_table
    bounds = PC.bounds_for(L, t, measure)
    d, keep = taken(K, t, measure, bounds)
    text = K.Distance(measure, PC.K_LEN, t["counts"] & DC.M32, filters=bounds, sparse_in=True, sparse_out=True)
    got, rc = text.rows(t["text"])
    assert rc == 0 and got == d.csr_rows(0, PC.NR) == PC.witness(L, t, measure, bounds)
    d.close()
    text.close()


@pytest.mark.gpu
def test_a_second_handle_borrows_the_csr(K, L, main_table):
    t = main_table
    first, keep = taken(K, t, "jaccard")
    rp, co, va, nr = first.csr_ptrs()
    assert (rp, co, va, nr) == keep.ptrs() + (PC.NR,)
    bounds = PC.bounds_for(L, t, "ani")
    second = handle(K, t, "ani", bounds)
    second.take_csr(rp, co, va, nr, t["row_counts"], t["row_names"])
    assert second.csr_rows(0, PC.NR) == PC.witness(L, t, "ani", bounds)
    assert first.csr_rows(0, PC.NR) == PC.witness(L, t, "jaccard")
    first.close()
    second.close()


@pytest.mark.gpu
def test_refusals(K, L, main_table, golden_dir):
    t = main_table
    keep = Dev(t["ptr"], t["col"], t["val"])
    for flags, word in (({"triangle": True, "sparse_out": True}, "KMDB_DISTANCE_TRIANGLE"), ({"sparse_in": True, "sparse_out": True}, "KMDB_DISTANCE_SPARSE_IN"),
                        ({"phylip": True, "sparse_out": True}, "KMDB_DISTANCE_PHYLIP"), ({}, "KMDB_DISTANCE_SPARSE_OUT")):
        d = K.Distance("jaccard", PC.K_LEN, t["counts"], **flags)
        with pytest.raises(K.KmdbError, match="kmdb_distance_take_csr_device.*" + word):
            d.take_csr(*keep.ptrs(), PC.NR, t["row_counts"], t["row_names"])
        with pytest.raises(K.KmdbError, match="kmdb_distance_parts_begin_rows.*" + word):
            d.parts_begin(t["row_counts"], t["row_names"])
        with pytest.raises(K.KmdbError, match="kmdb_distance_csr_rows.*" + word):
            d.csr_rows(0, 1)
        d.close()
    d = handle(K, t, "num-kmers")
    with pytest.raises(K.KmdbError, match="kmdb_distance_csr_rows: no CSR was taken"):
        d.csr_rows(0, 1)
    with pytest.raises(K.KmdbError, match="kmdb_distance_csr_device: no CSR was taken"):
        d.csr_ptrs()
    d.take_csr(*keep.ptrs(), PC.NR, t["row_counts"], t["row_names"])
    with pytest.raises(K.KmdbError, match="kmdb_distance_csr_rows: row_hi 13 > 12"):
        d.csr_rows(0, 13)
    with pytest.raises(K.KmdbError, match="kmdb_distance_csr_rows: row_lo > row_hi"):
        d.csr_rows(2, 1)
    assert d.csr_rows(1, 2) == PC.witness(L, t, "num-kmers", rows=(1, 2))      # the handle stays usable
    with pytest.raises(K.KmdbError, match="kmdb_distance_take_csr_device: .*entries and a null pointer"):
        d.take_csr(keep.ptr.data_ptr(), None, None, PC.NR, t["row_counts"], t["row_names"])
    with pytest.raises(K.KmdbError, match="kmdb_distance_csr_rows: no CSR was taken"):      # a refused take leaves nothing behind
        d.csr_rows(0, 1)
    # a column >= n and a row_ptr that descends: found on the device, refused with a message
    bad_col = t["col"].copy()
    bad_col[100] = 200
    bad = Dev(t["ptr"], bad_col, t["val"])
    with pytest.raises(K.KmdbError, match=r"kmdb_distance_take_csr_device: a column of the CSR \(200\) is not below the 200 columns"):
        d.take_csr(*bad.ptrs(), PC.NR, t["row_counts"], t["row_names"])
    bad_ptr = t["ptr"].copy()
    bad_ptr[3], bad_ptr[4] = bad_ptr[4], bad_ptr[3]
    bad = Dev(bad_ptr, t["col"], t["val"])
    with pytest.raises(K.KmdbError, match="kmdb_distance_take_csr_device: row_ptr does not ascend"):
        d.take_csr(*bad.ptrs(), PC.NR, t["row_counts"], t["row_names"])
    # the adds: no open block row, a part that does not fit the columns, a query shard, the wrong row database
    path = os.path.join(golden_dir, "synth_k21.db")                  # five samples
    h = K.HostDB(path)
    db = K.DeviceDB(h, with_hashtables=True)
    with pytest.raises(K.KmdbError, match="kmdb_distance_parts_add_all2all: no block row is open"):
        d.parts_add_all2all(db, 0)
    d.parts_begin(t["row_counts"][:5], t["row_names"][:5])
    with pytest.raises(K.KmdbError, match="kmdb_distance_parts_add_all2all: col_shift 196 \\+ 5 samples lie behind the 200 columns"):
        d.parts_add_all2all(db, 196)
    shard = K.DeviceDB(h, query_shard=(0, 2))
    with pytest.raises(K.KmdbError, match="kmdb_distance_parts_add_db2db: a query shard"):
        d.parts_add_db2db(db, shard, 0)
    shard.close()
    with pytest.raises(K.KmdbError, match=r"kmdb_distance_parts_add_csr_device: a column of the cell \(200\) is not below its 200 columns"):
        d.parts_add_csr(*Dev(np.arange(6, dtype=np.uint64), np.array([1, 2, 200, 4, 5], np.uint32), np.ones(5, np.uint32)).ptrs(), 200, 0)
    d.parts_begin(t["row_counts"][:4], t["row_names"][:4])
    with pytest.raises(K.KmdbError, match="kmdb_distance_parts_add_all2all: the row database holds 5 samples, the block row was begun with 4"):
        d.parts_add_all2all(db, 0)
    d.parts_begin(t["row_counts"][:5], t["row_names"][:5])           # and the handle serves a part that fits it
    d.parts_add_all2all(db, 0)
    assert d.csr_rows(0, 5).count(b"\n") == 5
    with pytest.raises(K.KmdbError, match="kmdb_distance_parts_add_all2all: no block row is open"):      # the rows asked for closed it
        d.parts_add_all2all(db, 0)
    d.close()
    db.close()


# ---- the gather ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_gather_is_the_concatenation(K, L, main_table):
    cells = PC.gather_cells()
    ptr, col, val = PC.gathered(cells)
    counts = main_table["counts"]
    g = PC.finish(PC.N, PC.NR, PC.ROW0, counts, ptr, col, val)
    d = handle(K, g, "num-kmers")
    d.parts_begin(g["row_counts"], g["row_names"])
    keep = []
    for p, c, v, w, shift in cells:
        keep.append(Dev(p, c, v))
        d.parts_add_csr(*keep[-1].ptrs(), w, shift)
    del keep                                                         # (the cells were copied in)
    assert d.csr_row_ptr().tolist() == ptr.tolist()
    rows = PC.parse_rows(d.csr_rows(0, PC.NR))
    assert [nm for nm, _ in rows] == g["row_names"]
    got_col = [c for _, r in rows for c, _ in r]
    got_val = [int(float(x)) for _, r in rows for _, x in r]
    assert got_col == col.tolist() and got_val == val.tolist()
    st = d.parts_stats()
    assert st["block_rows"] == 1 and st["grid_cells"] == 5 and st["cells_in"] == len(col) == st["cells_written"] + st["host_cells"], st
    assert st["peak_bytes"] >= 2 * (8 * len(col) + 8 * (PC.NR + 1)) and st["gather_ms"] > 0, st
    # a second handle borrows the gathered CSR; the next block row drops it
    second = handle(K, g, "jaccard")
    second.take_csr(*d.csr_ptrs(), g["row_counts"], g["row_names"])
    assert second.csr_rows(0, PC.NR) == PC.witness(L, g, "jaccard")
    second.close()
    d.parts_begin(g["row_counts"], g["row_names"])                   # a block row without a single cell: twelve empty rows
    assert d.csr_rows(0, PC.NR) == b"".join(nm + b",\n" for nm in g["row_names"])
    d.close()


@pytest.mark.gpu
def test_the_gather_of_one_long_row_among_many_empty_ones(K):
    """one row of 10^5 entries among 10^5 rows without any, from two cells of 60 000 and 40 001 columns: what a gather that walked rows, or
    spent a wave on every row, would make slow, and what puts the search of row_ptr, the copy and the names on many workgroups.  num-kmers:
    the text of a value is the count itself, so the witness is numpy and string formatting alone."""
    nr, widths, long_row = 100_001, (60_000, 40_001), 70_000
    n = sum(widths)
    rng = np.random.default_rng(8)
    counts = rng.integers(3_000_000, 6_000_000, n)
    names = PC.names_of(nr)
    d = K.Distance("num-kmers", PC.K_LEN, counts, sparse_out=True)
    d.parts_begin(rng.integers(3_000_000, 6_000_000, nr), names)
    want_col, want_val, shift = [], [], 0
    for w, held in zip(widths, (60_000, 40_000)):
        ptr = np.zeros(nr + 1, np.uint64)
        ptr[long_row + 1:] = held
        col, val = np.arange(held, dtype=np.uint32), rng.integers(1, 1 << 20, held).astype(np.uint32)
        cell = Dev(ptr, col, val)
        d.parts_add_csr(*cell.ptrs(), w, shift)
        want_col.append(col.astype(np.int64) + shift)
        want_val.append(val)
        shift += w
    del cell
    merged = d.csr_row_ptr()
    assert merged[long_row] == 0 and merged[long_row + 1] == merged[-1] == 100_000
    row = b"".join(b"%d:%d.000000," % (c + 1, v) for c, v in zip(np.concatenate(want_col).tolist(), np.concatenate(want_val).tolist()))
    want = b"".join(nm + b"," + (row if r == long_row else b"") + b"\n" for r, nm in enumerate(names))
    assert d.csr_rows(0, nr) == want
    assert d.csr_rows(long_row - 1, long_row + 2) == names[long_row - 1] + b",\n" + names[long_row] + b"," + row + b"\n" + names[long_row + 1] + b",\n"
    st = d.parts_stats()
    assert st["cells_in"] == st["cells_written"] // 2 == 100_000 and st["host_cells"] == 0, st
    d.close()


# ---- real cells ---------------------------------------------------------------------------------------------------------------------------------
def csr_text(names, row_counts, pieces):
    """the sparse rows of a block row as all2all-parts writes them: per row the entries of its cells in order, the columns shifted"""
    out = []
    for r, nm in enumerate(names):
        row = [nm + b",%d," % row_counts[r]]
        for sp, shift in pieces:
            for e in range(int(sp.row_ptr[r]), int(sp.row_ptr[r + 1])):
                row.append(b"%d:%d," % (int(sp.col[e]) + shift + 1, int(sp.val[e])))
        out.append(b"".join(row) + b"\n")
    return b"".join(out)


@pytest.mark.gpu
@pytest.mark.parametrize("measure,bounds", [("jaccard", []), ("mash", [("mash", None, 0.2), ("num-kmers", 100, None)])], ids=["jaccard", "mash-bounded"])
def test_a_grid_of_three_parts(K, L, grid3, measure, bounds):
    g = grid3
    n, N = 30, 90
    names = PC.names_of(N)
    counts = g["all_kmers"].astype(np.int64)
    other, lo, hi = PC.split_bounds(bounds)
    d = K.Distance(measure, g["k"], counts, filters=bounds, sparse_out=True)
    borrower = K.Distance("max", g["k"], counts, sparse_out=True)
    cache = {}
    total = 0
    for i in range(3):
        rk, rn = g["kmers"][i], names[i * n:(i + 1) * n]
        d.parts_begin(rk, rn)
        pieces = []
        for j in range(i):
            d.parts_add_db2db(g["parts"][i], g["parts"][j], j * n)
            pieces.append((g["parts"][i].db2db_sparse(g["parts"][j]), j * n))
        d.parts_add_all2all(g["parts"][i], i * n)
        pieces.append((g["parts"][i].all2all_sparse(), i * n))
        text = csr_text(rn, [int(x) for x in rk], pieces)
        total += text.count(b":")
        want = DC.Rules(L, measure, g["k"], counts, bounds=other, kmer_lo=lo, kmer_hi=hi, sparse_out=True, triangle=False, cache=cache).rows(text)
        assert d.csr_rows(0, n) == want, i
        assert d.csr_rows(0, 7) + d.csr_rows(7, n) == want, i
        borrower.take_csr(*d.csr_ptrs(), rk, rn)
        assert borrower.csr_rows(0, n) == DC.Rules(L, "max", g["k"], counts, sparse_out=True, triangle=False, cache=cache).rows(text), i
    st = d.parts_stats()
    assert st["block_rows"] == 3 and st["grid_cells"] == 6 and st["cells_in"] == total and total > N, st
    d.close()
    borrower.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def run_parts(tmp_path, golden_dir, opts, env_extra=None, name="out"):
    lst, out = tmp_path / "db.list", tmp_path / name
    lst.write_text(os.path.join(golden_dir, "virus_k18_part1.db") + "\n" + os.path.join(golden_dir, "virus_k18_part2.db") + "\n")
    r = cli(["all2all-parts"] + opts + [lst, out], dict(env_extra or {}, KMDB_VERBOSE="1"))
    assert r.returncode == 0, r.stderr
    return out, r.stderr


def host_distance(tmp_path, golden_dir, opts, measure):
    want = tmp_path / "want"
    r = cli(["distance", "-host", "-sparse"] + opts + [measure, os.path.join(golden_dir, "virus.k18.sparse.csv"), want])
    assert r.returncode == 0, r.stderr
    return want.read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("opts,measure", [([], "jaccard"), (["-min", "0.0", "-max", "0.3"], "mash"), (["-min", "0.99", "-min", "num-kmers:29000"], "jaccard")],
                         ids=["jaccard", "mash-bounded", "jaccard-cut"])
def test_cli_virus_parts(L, golden_dir, tmp_path, opts, measure):
    want = host_distance(tmp_path, golden_dir, opts, measure)
    assert want == DC.distance_file(L, open(os.path.join(golden_dir, "virus.k18.sparse.csv"), "rb").read(), ["-sparse"] + opts + [measure])
    pairs = want.count(b":") - 2                                      # (the header line holds two)
    assert 0 < pairs < 13530 if "0.99" in opts else pairs == 13530   # 165 samples: the bounds of the third case cut, the others keep every pair
    out, err = run_parts(tmp_path, golden_dir, opts + ["-distance", measure])
    assert out.read_bytes() == want
    m = re.search(r"distance from the grid, worker 0: block rows (\d+), cells (\d+), entries in (\d+)", err)
    assert (int(m.group(1)), int(m.group(2))) == (2, 3), err
    whole = tmp_path / "whole"                                       # all2all-sp -distance on the whole collection: same header, same rows
    r = cli(["all2all-sp"] + opts + ["-distance", measure, os.path.join(golden_dir, "virus_k18.db"), whole])
    assert r.returncode == 0 and whole.read_bytes() == want, r.stderr
    out, err = run_parts(tmp_path, golden_dir, opts + ["-sparse", "-gpus", "2", "-distance", measure], name="out.g2")
    assert out.read_bytes() == want and "dealt to 2 workers" in err
    out, err = run_parts(tmp_path, golden_dir, opts + ["-distance", measure], {"KMDB_DISTANCE_CELLS_PER_PIECE": "50"}, "out.50")
    assert out.read_bytes() == want


@pytest.mark.gpu
def test_cli_several_measures_share_one_pass(golden_dir, tmp_path):
    out, err = run_parts(tmp_path, golden_dir, ["-min", "0.995", "-distance", "jaccard", "-distance", "max"])
    assert not out.exists()
    for measure in ("jaccard", "max"):                               # the bare bound belongs to the measure of each table
        want = host_distance(tmp_path, golden_dir, ["-min", "0.995"], measure)
        assert (tmp_path / ("out." + measure)).read_bytes() == want and 10 < want.count(b":") < 13000, measure
    assert err.count("Processing cell") == 3
