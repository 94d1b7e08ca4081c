"""kmdb_db2db_sparse_filtered: the cell of two databases compacted and filtered on the device — db2db_sp + SparseMatrix::compact2 with the
-min / -max CombinedFilter (reference src/console_all2all_parts.cpp:179-195, 225-241) — and all2all-parts on top of it.  Expected values never
come from kmdb_db2db_dense: they are the reference's recorded output (tests/golden), the CPU oracle's dense cell, and kmdbh_metric with
a = the ROW sample's k-mer count and b = the COLUMN sample's."""
import ctypes
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ENTRY = "kmdb_db2db_sparse_filtered"
FMAX = float(np.finfo(np.float64).max)


def mash_of(q, k):
    """the mash distance of a ratio q (reference src/params.cpp:14-42): -(1/k) ln(2 q / (1 + q))"""
    return -math.log(2.0 * q / (1.0 + q)) / k


# ------------------------------------------------------------------------------------------------ CPU
def test_abi_is_additive(K):
    """1. both entry points are exported and declared, the header announces them, the ABI version stays 8"""
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    for name in (ENTRY, "kmdb_db2db_stats_get"):
        assert name in K.capi.EXPORTS and name + "(" in header and hasattr(L, name), name
    assert "#define KMDB_HAS_DB2DB_SPARSE 1" in header
    assert L.kmdb_abi_version() == 8 and K.capi.ABI_VERSION == 8


def test_argument_checks_come_before_any_device_work(K):
    """2. null handles are refused with the entry point's name; so are — with handles that are never looked at — filters or a measure without both
    count arrays, an unknown metric or measure and too many bounds"""
    L = K.lib()
    raw = K.capi._Sparse()
    assert L.kmdb_db2db_sparse_filtered(None, None, None, 0, None, None, -1, ctypes.byref(raw), None) != 0
    assert ENTRY in L.kmdb_last_error().decode()
    fake = ctypes.create_string_buffer(1 << 16)                  # stands for a handle: a call refused on its arguments never reads it
    h = ctypes.cast(fake, ctypes.c_void_p)
    assert L.kmdb_db2db_sparse_filtered(h, h, None, 0, None, None, -1, None, None) != 0 and ENTRY in L.kmdb_last_error().decode()
    assert L.kmdb_db2db_stats_get(None, None) != 0 and "kmdb_db2db_stats_get" in L.kmdb_last_error().decode()
    cnt = np.ones(4, np.uint32)
    one = K.capi._filters([("jaccard", 0.5, None)])
    bad = K.capi._filters([("jaccard", 0.5, None)])
    bad[0].metric = 99
    many = K.capi._filters([("jaccard", 0.0, None)] * 13)
    cases = [(one, 1, None, None, -1, "null argument"), (one, 1, cnt.ctypes.data, None, -1, "null argument"), (one, 1, None, cnt.ctypes.data, -1, "null argument"),
             (None, 0, cnt.ctypes.data, None, 5, "null argument"), (None, 0, cnt.ctypes.data, cnt.ctypes.data, 99, "unknown measure"),
             (bad, 1, cnt.ctypes.data, cnt.ctypes.data, -1, "unknown metric"), (many, 13, cnt.ctypes.data, cnt.ctypes.data, -1, "more than 12 bounds")]
    for fs, n, rk, ck, measure, what in cases:
        assert L.kmdb_db2db_sparse_filtered(h, h, fs, n, rk, ck, measure, ctypes.byref(raw), None) != 0, what
        msg = L.kmdb_last_error().decode()
        assert msg.startswith(ENTRY + ":") and what in msg, msg


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def S(K):
    return importlib.import_module("kmerdb_amd.synth")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


def _synth_part(S, g, ids, k, path, device):
    """database (with hashtables) of the samples `ids` of the genome model g, written in kmer-db's format"""
    pat = S.build_patterns(lambda i: S.kmers_of(g.sample(ids[i]), k), len(ids), device)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    S.write_db(path, k, 1.0, [g.name(i) for i in ids], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)


class Cell:
    """two resident parts (rows x columns), their k-mer counts and the ORACLE's dense cell, computed once and never written to"""

    def __init__(self, K, O, dev, p_row, p_col):
        hr, hc = K.HostDB(p_row), K.HostDB(p_col)
        self.k = hr.k
        self.a, self.b = hr.sample_kmers.astype(np.uint32), hc.sample_kmers.astype(np.uint32)
        self.drow = K.DeviceDB(hr, device=dev, with_hashtables=True)
        self.dcol = K.DeviceDB(hc, device=dev, with_hashtables=True)
        self.orow, self.ocol = O.OracleDB(p_row), O.OracleDB(p_col)
        self.dense = self.orow.db2db(self.ocol)
        self.dense.setflags(write=False)


def synth_cell(K, O, S, dev, tmp, tag, g_args, rows, cols, k=18):
    import torch
    device = torch.device("cuda", dev)
    g = S.CladeGenomes(*g_args[0], device=device, **g_args[1])
    pr, pc = str(tmp / (tag + "_rows.db")), str(tmp / (tag + "_cols.db"))
    _synth_part(S, g, rows, k, pr, device)
    _synth_part(S, g, cols, k, pc, device)
    return Cell(K, O, dev, pr, pc)


@pytest.fixture(scope="module")
def virus(K, O, golden_dir, dev):
    """virus_k18_part2 x virus_k18_part1: 65 x 100, completely dense; row 64 sits alone in the second row block"""
    return Cell(K, O, dev, os.path.join(golden_dir, "virus_k18_part2.db"), os.path.join(golden_dir, "virus_k18_part1.db"))


@pytest.fixture(scope="module")
def clade75(K, O, S, dev, tmp_path_factory):
    """CladeGenomes(300, 50, 1500, r1=0.75): rows = odd ids, columns = even ids — 150 x 150, 3 x 3 tiles, a last block of 22, clades that share nothing"""
    return synth_cell(K, O, S, dev, tmp_path_factory.mktemp("c75"), "il", ((300, 50, 1500), dict(r1=0.75, r2=0.01, seed=11)),
                      list(range(1, 300, 2)), list(range(0, 300, 2)))


def rows_of(sp):
    return [list(zip(*(a.tolist() for a in sp.row(i)))) for i in range(sp.n_rows)]


def nonzeros(dense, keep=None):
    """the rows (col, val) of a dense cell, ascending columns; keep: a boolean mask of the cells to list"""
    m = dense != 0 if keep is None else (dense != 0) & keep
    return [[(int(c), int(dense[r, c])) for c in np.flatnonzero(m[r])] for r in range(dense.shape[0])]


def touched_tiles(dense):
    nr, nc = dense.shape
    return sum(1 for X in range(0, nr, 64) for Y in range(0, nc, 64) if dense[X:X + 64, Y:Y + 64].any())


def metric_cells(K, name, dense, a, b, k):
    """kmdbh_metric of every non-zero cell with the ROW sample's count first (NaN where the cell is zero)"""
    L = K.lib()
    m = K.capi.METRICS.index(name)
    out = np.full(dense.shape, np.nan)
    for r, c in zip(*np.nonzero(dense)):
        out[r, c] = L.kmdbh_metric(m, int(dense[r, c]), int(a[r]), int(b[c]), int(k))
    return out


def expected_keep(K, cell, filters, swap=False):
    """the cells that pass every bound, decided by kmdbh_metric on the oracle's cell; swap: with the column sample's count as a (the WRONG order)"""
    a, b = (cell.a, cell.b)
    keep = cell.dense != 0
    for name, lo, hi in filters:
        if swap:
            x = metric_cells(K, name, cell.dense.T, b, a, cell.k).T
        else:
            x = metric_cells(K, name, cell.dense, a, b, cell.k)
        with np.errstate(invalid="ignore"):
            keep &= (x >= (-FMAX if lo is None else lo)) & (x <= (FMAX if hi is None else hi))
    return keep


def check_filtered(K, cell, filters, measure=None):
    """the call with these bounds == the expected set, which keeps at least one and drops at least one non-zero cell"""
    keep = expected_keep(K, cell, filters)
    n_keep, n_nz = int(keep.sum()), int((cell.dense != 0).sum())
    print("%s: keeps %d of %d" % (filters, n_keep, n_nz))
    assert 0 < n_keep < n_nz, "vacuous bound %s: keeps %d of %d" % (filters, n_keep, n_nz)
    sp = cell.drow.db2db_sparse(cell.dcol, filters, cell.a, cell.b, measure=measure)
    assert rows_of(sp) == nonzeros(cell.dense, keep), filters
    st = cell.drow.db2db_stats()
    assert st["nnz"] == n_keep == sp.nnz and st["nnz_device"] >= st["nnz"] and st["nnz_device"] <= n_nz
    assert st["d2h_bytes"] == 8 * (cell.dense.shape[0] + 1) + 8 * st["nnz_device"]
    return sp, keep


@pytest.mark.gpu
def test_the_references_own_cell(K, O, golden_dir, virus, tmp_path):
    """3. virus part 2 x part 1 rendered as the reference writes it == the reference's recorded db2db_sp + compact2, line for line; == the oracle's
    non-zeros; the transposed call; a database against itself (the full square, diagonal included)"""
    sp = virus.drow.db2db_sparse(virus.dcol)
    assert sp.n_rows == 65 and sp.measure is None and sp.nnz == 6500
    want = open(os.path.join(golden_dir, "virus_k18_part2_x_part1.db2db_sp.ref.txt"), "rb").read()
    got = b"".join("".join("%d:%d," % (c + 1, v) for c, v in row).encode() + b"\n" for row in rows_of(sp))
    assert got.split(b"\n") == want.split(b"\n")
    assert rows_of(sp) == nonzeros(virus.dense)
    if O.have_ref():
        p2, p1 = os.path.join(golden_dir, "virus_k18_part2.db"), os.path.join(golden_dir, "virus_k18_part1.db")
        assert O.ref_db2db_sp(p2, p1, str(tmp_path / "ref.txt"), threads=2)[0] == got
    st = virus.drow.db2db_stats()
    assert st["tiles"] == 4 and st["tiles_touched"] == 4 and st["nnz_device"] == st["nnz"] == 6500 and st["d2h_bytes"] == 8 * 66 + 8 * 6500
    assert st["compact_ms"] > 0
    assert rows_of(virus.dcol.db2db_sparse(virus.drow)) == nonzeros(virus.dense.T)
    assert rows_of(virus.dcol.db2db_sparse(virus.dcol)) == nonzeros(virus.ocol.db2db(virus.ocol))


@pytest.mark.gpu
def test_untouched_tiles_and_partial_blocks(K, O, S, dev, clade75, tmp_path, monkeypatch):
    """4. 150 x 150 in 3 x 3 tiles with a last block of 22 and tiles that receive nothing: only the touched tiles are read; KMDB_SP_ALL_TILES=1
    reads all of them and returns the same rows; two parts without a shared clade give an empty CSR without a scan"""
    c = clade75
    assert c.dense.shape == (150, 150)
    want, tt = nonzeros(c.dense), touched_tiles(c.dense)
    print("non-zero cells %d, touched tiles %d of 9" % (int((c.dense != 0).sum()), tt))
    sp = c.drow.db2db_sparse(c.dcol)
    assert rows_of(sp) == want
    st = c.drow.db2db_stats()
    assert st["tiles"] == 9 and st["tiles_touched"] == tt and 0 < st["tiles_touched"] < st["tiles"]
    assert st["d2h_bytes"] < 4 * 150 * 150 and st["nnz"] == st["nnz_device"] == sp.nnz
    monkeypatch.setenv("KMDB_SP_ALL_TILES", "1")
    assert rows_of(c.drow.db2db_sparse(c.dcol)) == want
    st = c.drow.db2db_stats()
    assert st["tiles_touched"] == st["tiles"] == 9
    monkeypatch.delenv("KMDB_SP_ALL_TILES")
    # the dense entry on the same handle: its own numbers
    c.drow.db2db(c.dcol)
    st = c.drow.db2db_stats()
    assert st["tiles"] == 9 and st["tiles_touched"] == 0 and st["d2h_bytes"] == 4 * 150 * 150
    # halves: rows = ids 150 .. 299, columns = 0 .. 149 share no clade
    h = synth_cell(K, O, S, dev, tmp_path, "halves", ((300, 50, 1500), dict(r1=0.75, r2=0.01, seed=11)), list(range(150, 300)), list(range(150)))
    sp = h.drow.db2db_sparse(h.dcol)
    assert rows_of(sp) == nonzeros(h.dense)
    st = h.drow.db2db_stats()
    assert st["tiles_touched"] == touched_tiles(h.dense)
    if not h.dense.any():
        assert sp.nnz == 0 and not sp.row_ptr.any() and st["tiles_touched"] == 0 and st["tiles"] == 9


@pytest.mark.gpu
def test_more_than_64_column_blocks(K, O, S, dev, tmp_path):
    """5. 132 x 4198 = 3 x 66 tiles: the flag loop of a row takes a second round, and touched tiles lie in column blocks 64 and 65"""
    rows = list(range(0, 4330, 33))
    rs = set(rows)
    cols = [i for i in range(4330) if i not in rs]
    c = synth_cell(K, O, S, dev, tmp_path, "wide", ((4330, 50, 300), dict(r1=0.75, r2=0.01, seed=11)), rows, cols)
    assert c.dense.shape == (132, 4198)
    tt = touched_tiles(c.dense)
    print("non-zero cells %d, touched tiles %d of 198, of them beyond column block 63: %d" % (int((c.dense != 0).sum()), tt, touched_tiles(c.dense[:, 4096:])))
    sp = c.drow.db2db_sparse(c.dcol)
    assert rows_of(sp) == nonzeros(c.dense)
    assert sp.nnz and int(sp.col.max()) >= 4096
    st = c.drow.db2db_stats()
    assert st["tiles"] == 198 and st["tiles_touched"] == tt and 0 < st["tiles_touched"] < st["tiles"]


@pytest.mark.gpu
def test_bounds_and_measures_row_sample_first(K, O, S, dev, virus, tmp_path):
    """6. every bound against kmdbh_metric(metric, c, a = row count, b = column count, k) on the oracle's cell; the virus samples' counts differ, so
    mash-query tells the row sample from the column sample"""
    v = virus
    mq = mash_of(0.995, 18)
    check_filtered(K, v, [("jaccard", 0.99, None)])
    check_filtered(K, v, [("num-kmers", 29600.0, 29750.0)])
    sp, keep = check_filtered(K, v, [("mash-query", None, mq)])
    swapped = expected_keep(K, v, [("mash-query", None, mq)], swap=True)
    print("mash-query: %d with the row sample as a, %d with the sides swapped, %d cells differ" % (int(keep.sum()), int(swapped.sum()), int((keep != swapped).sum())))
    assert (keep != swapped).any(), "the cell cannot tell the row sample from the column sample"
    # ani >= and max <= together; thresholds inside the observed range: the medians of the two measures over the cell
    ani = metric_cells(K, "ani", v.dense, v.a, v.b, v.k)
    mx = metric_cells(K, "max", v.dense, v.a, v.b, v.k)
    t_ani, t_max = float(np.nanmedian(ani)), float(np.nanquantile(mx, 0.75))
    sp, keep = check_filtered(K, v, [("ani", t_ani, None), ("max", None, t_max)], measure="ani")
    # the measures: bit-equal to kmdbh_metric
    want = np.array([ani[r, c] for r in range(65) for c in np.flatnonzero(keep[r])])
    assert sp.measure is not None and sp.measure.tobytes() == want.tobytes()
    sp = v.drow.db2db_sparse(v.dcol, (), v.a, v.b, measure="mash-query")
    mqs = metric_cells(K, "mash-query", v.dense, v.a, v.b, v.k)
    assert sp.nnz == 6500 and sp.measure.tobytes() == mqs.reshape(-1).tobytes()
    # a bound placed exactly on one cell's value keeps that cell (the margin band and the host's decision), from either side
    jac = metric_cells(K, "jaccard", v.dense, v.a, v.b, v.k)
    for r, c in ((64, 99), (0, 0), (31, 57)):
        for fl in ([("jaccard", float(jac[r, c]), None)], [("jaccard", None, float(jac[r, c]))], [("ani", float(ani[r, c]), None)],
                   [("mash-query", None, float(mqs[r, c]))]):
            got = rows_of(v.drow.db2db_sparse(v.dcol, fl, v.a, v.b))
            assert (c, int(v.dense[r, c])) in got[r], (r, c, fl)
            assert got == nonzeros(v.dense, expected_keep(K, v, fl)), (r, c, fl)
    # a cell with jaccard from 3e-4 to 0.75: bounds that cut deep into it
    w = synth_cell(K, O, S, dev, tmp_path, "r10", ((300, 50, 1500), dict(r1=0.10, r2=0.01, seed=11)), list(range(1, 300, 2)), list(range(0, 300, 2)))
    jw = metric_cells(K, "jaccard", w.dense, w.a, w.b, w.k)
    print("r1 = 0.10: %d non-zero cells, jaccard %.3g .. %.3g" % (int((w.dense != 0).sum()), float(np.nanmin(jw)), float(np.nanmax(jw))))
    check_filtered(K, w, [("jaccard", 0.3, None)])
    check_filtered(K, w, [("mash", None, 0.05)])
    check_filtered(K, w, [("num-kmers", float(np.median(w.dense[w.dense != 0])) + 0.5, None)])
    check_filtered(K, w, [("mash-query", None, mash_of(0.5, 18))])
    aw, mw = metric_cells(K, "ani", w.dense, w.a, w.b, w.k), metric_cells(K, "max", w.dense, w.a, w.b, w.k)
    check_filtered(K, w, [("ani", float(np.nanquantile(aw, 0.25)), None), ("max", None, float(np.nanquantile(mw, 0.9)))])


def _cli(*args, env=None):
    exe = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=None if env is None else dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.gpu
def test_front_end_filters_on_the_device(K, golden_dir, dev, tmp_path):
    """7. all2all-parts over the two virus parts with a bound == the rows of the reference's unfiltered output (golden virus.k18.sparse.csv) with every
    col:val kept or dropped by kmdbh_metric and the k-mer counts of the file's second line; the same bytes with dense cells and with -gpus 2"""
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    L = K.lib()
    lines = open(g("virus.k18.sparse.csv"), "rb").read().split(b"\n")
    counts = [int(x) for x in lines[1].split(b",")[2:] if x]
    assert lines[1].startswith(b"query-samples,total-kmers,") and len(counts) == 165
    with open(t("db.list"), "w") as f:
        f.write(g("virus_k18_part1.db") + "\n" + g("virus_k18_part2.db") + "\n")
    mq = mash_of(0.995, 18)
    for tag, opt, metric, lo, hi in (("minj", ["-min", "jaccard:0.99"], "jaccard", 0.99, FMAX), ("maxq", ["-max", "mash-query:%r" % mq], "mash-query", -FMAX, mq)):
        m = K.capi.METRICS.index(metric)
        want, kept, seen = lines[:2], 0, 0
        for i, ln in enumerate(lines[2:]):
            if not ln:
                want.append(ln)
                continue
            f = ln.split(b",")
            cells = []
            for cv in f[2:-1]:
                c, v = (int(x) for x in cv.split(b":"))
                seen += 1
                if lo <= L.kmdbh_metric(m, v, counts[i], counts[c - 1], 18) <= hi:
                    cells.append(cv)
            kept += len(cells)
            want.append(b",".join(f[:2] + cells + [b""]))
        print("%s: keeps %d of %d pairs" % (tag, kept, seen))
        assert 0 < kept < seen
        want = b"\n".join(want)
        outs = []
        for name, extra, env in (("sp", [], None), ("dense", [], {"KMDB_PARTS_DENSE_CELLS": "1"}), ("g2", ["-gpus", "2"], None),
                                 ("g2dense", ["-gpus", "2"], {"KMDB_PARTS_DENSE_CELLS": "1"})):
            out = t("%s.%s.csv" % (tag, name))
            _cli("all2all-parts", *opt, *extra, t("db.list"), out, env=env)
            outs.append(open(out, "rb").read())
        assert outs[0] == want, tag
        assert outs[1] == outs[0] and outs[2] == outs[0] and outs[3] == outs[0], tag
    _cli("all2all-parts", t("db.list"), t("plain.csv"))
    assert open(t("plain.csv"), "rb").read() == open(g("virus.k18.sparse.csv"), "rb").read()


@pytest.mark.gpu
def test_refusals_on_the_device(K, golden_dir, dev, virus):
    """8. what kmdb_db2db_dense refuses, under this entry point's name"""
    v = virus
    with pytest.raises(K.KmdbError, match=ENTRY + ": null argument"):
        v.drow.db2db_sparse(v.dcol, [("jaccard", 0.5, None)])
    with pytest.raises(K.KmdbError, match=ENTRY + ": null argument"):
        v.drow.db2db_sparse(v.dcol, (), v.a, None, measure="ani")
    with pytest.raises(K.KmdbError, match=ENTRY + ": both databases must be uploaded with hashtables"):
        v.drow.db2db_sparse(K.DeviceDB(K.HostDB(os.path.join(golden_dir, "virus_k18_part1.db"), skip_hashtables=True), device=dev))
    with pytest.raises(K.KmdbError, match=ENTRY + ": the databases have different k-mer lengths"):
        v.drow.db2db_sparse(K.DeviceDB(K.HostDB(os.path.join(golden_dir, "virus_k25_f01_part1.db")), device=dev, with_hashtables=True))
    # and the handle still serves
    assert v.drow.db2db_sparse(v.dcol).nnz == 6500
