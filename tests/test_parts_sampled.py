"""`all2all-parts -sample-rows <criterion>:<count>` with every cell's candidates selected on the device: the select of csrc/sample_rows.hip on a
RECTANGLE of two sample sets (kmdb_sampled_from_rect_device on the crafted rectangles of parts_sampled_cases.py), kmdb_db2db_sampled on real
cells, and the front-end on top of both.  Expected values never come from the code under test: they are the numpy restatement of the sampler's
rule over the rectangle (parts_sampled_cases.expected_rect), db.all2all_sampled on the whole collection (pinned to the reference's goldens by
test_sample_rows_device.py), or the reference's own goldens."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import parts_sampled_cases as C
from conftest import ROOT
from test_db2db_sparse import _synth_part, clade75, touched_tiles  # noqa: F401  (clade75: fixture)
from test_sample_rows_conformance import handle  # noqa: F401  (fixture)
from test_sample_rows_device import S, dev, golden_rows, rows_of  # noqa: F401  (S, dev: fixtures)

ENTRIES = ("kmdb_db2db_sampled", "kmdb_sampled_from_rect_device", "kmdb_db2db_sample_stats_get")
LINE = "sampled cell"                                   # the front-end's KMDB_VERBOSE line of a cell selected on the device


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_additive(K):
    """1. the three entry points are exported and declared, the header announces them, the ABI version stays 8"""
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    for name in ENTRIES:
        assert name in K.capi.EXPORTS and name + "(" in header and hasattr(L, name), name
    assert "#define KMDB_HAS_DB2DB_SAMPLED 1" in header
    assert L.kmdb_abi_version() == 8 and K.capi.ABI_VERSION == 8
    for name in ("db2db_sampled", "sampled_from_rect_device", "db2db_sample_stats"):
        assert hasattr(K.DeviceDB, name), name


def test_argument_checks_come_before_any_device_work(K):
    """2. refused under the entry's name with handles that are never looked at: NULL handles or outs, count 0, an unknown criterion, a missing
    count array (both are required, with or without filters), an unknown metric in a filter, more than 12 bounds; and for the rectangle entry
    nr + nc or a tile count beyond the select's 31-bit sizes"""
    L = K.lib()
    r1, r2 = K.capi._Sparse(), K.capi._Sparse()
    o1, o2 = ctypes.byref(r1), ctypes.byref(r2)
    fake = ctypes.create_string_buffer(1 << 16)                  # stands for a handle: a call refused on its arguments never reads it
    h = ctypes.cast(fake, ctypes.c_void_p)
    cnt = np.ones(4, np.uint32)
    p = cnt.ctypes.data
    one = K.capi._filters([("jaccard", 0.5, None)])
    bad = K.capi._filters([("jaccard", 0.5, None)])
    bad[0].metric = 99
    many = K.capi._filters([("jaccard", 0.0, None)] * 13)
    JAC = K.capi.METRICS.index("jaccard")

    def refused(rc, entry, what):
        msg = L.kmdb_last_error().decode()
        assert rc != 0 and msg.startswith(entry + ":") and what in msg, (entry, what, msg)

    e = ENTRIES[0]
    for hr, hc, a, b in ((None, h, o1, o2), (h, None, o1, o2), (h, h, None, o2), (h, h, o1, None)):
        refused(L.kmdb_db2db_sampled(hr, hc, None, 0, p, p, JAC, 3, a, b, None), e, "null argument")
    for fs, n, rk, ck, crit, count, what in ((None, 0, p, p, JAC, 0, "count must be at least 1"), (None, 0, p, p, 99, 3, "unknown criterion"),
                                             (None, 0, p, p, -1, 3, "unknown criterion"), (None, 0, None, p, JAC, 3, "sample_kmers is NULL"),
                                             (None, 0, p, None, JAC, 3, "sample_kmers is NULL"), (one, 1, None, None, JAC, 3, "sample_kmers is NULL"),
                                             (None, 1, p, p, JAC, 3, "null argument"), (bad, 1, p, p, JAC, 3, "unknown metric"),
                                             (many, 13, p, p, JAC, 3, "more than 12 bounds")):
        refused(L.kmdb_db2db_sampled(h, h, fs, n, rk, ck, crit, count, o1, o2, None), e, what)
        refused(L.kmdb_sampled_from_rect_device(h, h, 4, 4, fs, n, rk, ck, crit, count, o1, o2, None), ENTRIES[1], what)
    e = ENTRIES[1]
    for hd, a, b in ((None, o1, o2), (h, None, o2), (h, o1, None)):
        refused(L.kmdb_sampled_from_rect_device(hd, h, 4, 4, None, 0, p, p, JAC, 3, a, b, None), e, "null argument")
    refused(L.kmdb_sampled_from_rect_device(h, h, 1 << 30, 1 << 30, None, 0, p, p, JAC, 3, o1, o2, None), e, "samples in the two sets")
    refused(L.kmdb_sampled_from_rect_device(h, h, (1 << 31) - 3, 2, None, 0, p, p, JAC, 3, o1, o2, None), e, "samples in the two sets")
    refused(L.kmdb_sampled_from_rect_device(h, h, 1 << 29, 1 << 29, None, 0, p, p, JAC, 3, o1, o2, None), e, "tiles")
    refused(L.kmdb_db2db_sample_stats_get(None, None), ENTRIES[2], "null argument")
    refused(L.kmdb_db2db_sample_stats_get(h, None), ENTRIES[2], "null argument")


def test_the_cases_hold_what_they_are_named_for(K):
    """the digit cases settle their cut in the pass they are named for, on a row line and on a column line; the collapse case has fewer keys than
    cells and its cut inside one key; mash-query and max tell a from b on the 70 x 130 rectangle; the refetch bound sits one ulp above its cells"""
    for name in C.DIGIT_NAMES:
        c = C.case(name)
        count = c.runs[0][1]
        for vals in [C.line_values(c, row=r) for r in C.HUB_ROWS] + [C.line_values(c, col=x) for x in C.HUB_COLS]:
            keys = C.key_of(vals.astype(np.float64))
            if name == "collapse":
                ks = np.sort(keys)[::-1]
                assert len(np.unique(vals)) == 200 and len(np.unique(keys)) == 101 and ks[count - 1] == ks[count]
            else:
                assert len(vals) == len(C.DIGIT_VALUES[name][0]) and C.settle_digit(keys, count) == C.DIGIT_VALUES[name][2], name
    c = C.case("shape_70x130")
    swapped = C.Rect("swapped", c.nr, c.nc, 0, 0)
    swapped.cells = c.cells
    swapped.a, swapped.b = np.resize(c.b, c.nr), np.resize(c.a, c.nc)
    for criterion in ("mash-query", "max"):
        assert C.expected_rect(K, c, criterion, 5) != C.expected_rect(K, swapped, criterion, 5), criterion
    c = C.case("refetch")
    (_, _, ((_, bound, _),)), = c.runs
    j = C.metric_of(K, "jaccard", np.array([500, 500]), np.array([1000, 10_000]), np.array([10_000, 1000]), C.K_LEN)
    assert j[0] == j[1] < bound == np.nextafter(j[0], 2.0) and bound * (1 - C.WIDEN) < j[0]
    for cn in ("unrankable_row", "unrankable_col"):
        c = C.case(cn)
        assert len(C.unrankable_lines(c, "min")) > 3 and not C.unrankable_lines(c, "num-kmers") and not C.unrankable_lines(c, "jaccard")


class _Rows:
    """a (row_ptr, col, val) triple with the fields of a SparseRows, for global_part"""

    def __init__(self, n, lines):
        self.row_ptr = np.zeros(n + 1, np.uint64)
        self.row_ptr[1:] = np.cumsum([len(ln) for ln in lines])
        self.col = np.array([o for ln in lines for o, _ in ln], np.uint32)
        self.val = np.array([v for ln in lines for _, v in ln], np.uint32)


@pytest.mark.parametrize("name", ["shape_70x130", "unrankable_row", "unrankable_col", "refetch"])
def test_host_select_on_the_whole_rectangle(K, name):
    """kmdbh_sample_rows_select over the WHOLE rectangle as one part in global ids = the restated rule: pins the restatement, and that the
    collection's convention (the larger id is the row sample) scores a pair as the cell does (a = the row sample's count)"""
    c = C.case(name)
    rows = [sorted((x, v) for (r, x), v in c.cells.items() if r == s) for s in range(c.nr)]
    cols = [sorted((r, v) for (r, x), v in c.cells.items() if x == s) for s in range(c.nc)]
    part = C.global_part(c.nr, c.nc, _Rows(c.nr, rows), _Rows(c.nc, cols))
    for criterion, count, filters in c.runs:
        assert rows_of(K.sample_rows_select(criterion, count, C.K_LEN, c.kmers, [part], filters)) == C.expected_rect(K, c, criterion, count, filters), (criterion, count)


# ---- GPU: crafted rectangles ----------------------------------------------------------------------------------------------------------------
def upload(m):
    import torch
    return torch.from_numpy(np.array(m, np.uint32).view(np.int32)).cuda()


def lines_of(c, row_cand, col_cand):
    """the candidates per slot in global ids, after the checks every call must pass: n_rows, no measures, ascending distinct local ids inside
    the other set, values = the rectangle's"""
    assert row_cand.measure is None and col_cand.measure is None and row_cand.n_rows == c.nr and col_cand.n_rows == c.nc
    out = [None] * (c.nc + c.nr)
    for cand, n_other, first, shift, cell in ((row_cand, c.nc, c.nc, 0, lambda s, o: (s, o)), (col_cand, c.nr, 0, c.nc, lambda s, o: (o, s))):
        for s in range(cand.n_rows):
            ids, vals = cand.row(s)
            ids = ids.astype(np.int64)
            assert (np.diff(ids) > 0).all() and (not len(ids) or (ids[0] >= 0 and ids[-1] < n_other)), (c.name, first + s, ids)
            assert [c.cells.get(cell(s, int(o)), 0) for o in ids] == vals.tolist(), (c.name, first + s)
            out[first + s] = set((ids + shift).tolist())
    return out


def check_call(K, db, c, cells, criterion, count, filters=()):
    """both outputs are supersets of the exact best `count`, subsets of the non-zero cells that pass the widened bounds, ascending, with the
    matrix's values; merged by the host they give the restated rule exactly.  Returns (lines, the widened cells per slot, the stats)."""
    row_cand, col_cand = db.sampled_from_rect_device(cells.data_ptr(), c.nr, c.nc, criterion, count, c.a, c.b, filters)
    st = db.db2db_sample_stats()
    what = (c.name, criterion, count)
    want = C.expected_rect(K, c, criterion, count, filters)
    lines = lines_of(c, row_cand, col_cand)
    r, x, v = c.triplets()
    ok = C.widened_pass(r, x, v, c.a, c.b, filters)
    wide = [set() for _ in range(c.nc + c.nr)]
    for rr, xx in zip(r[ok].tolist(), x[ok].tolist()):
        wide[c.nc + rr].add(xx)
        wide[xx].add(c.nc + rr)
    for s in range(c.nc + c.nr):
        assert {o for o, _ in want[s]} <= lines[s] <= wide[s], what + (s,)
    part = C.global_part(c.nr, c.nc, row_cand, col_cand)
    assert rows_of(K.sample_rows_select(criterion, count, C.K_LEN, c.kmers, [part], filters)) == want, what
    assert st["candidates"] == row_cand.nnz + col_cand.nnz and st["triangle_reads"] >= 5, what
    return lines, wide, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.SHAPE_NAMES + ["column_edge"])
def test_shapes_and_the_column_edge(K, handle, name):
    """3. + 4. 1 x 1 to 130 x 70, counts 1, 5, 64 and one larger than nc, every criterion on 70 x 130 with unequal row and column counts; and the
    rectangle whose last column block is 6 columns wide beside the next row's largest cells"""
    c = C.case(name)
    db = handle(2)
    cells = upload(c.dense())
    for criterion, count, filters in c.runs:
        lines, wide, st = check_call(K, db, c, cells, criterion, count, filters)
        assert st["rows_refetched"] == 0
        if count > max(c.nr, c.nc):
            assert lines == wide and st["rows_truncated"] == 0
        if name == "column_edge" and criterion == "num-kmers":
            for r in range(c.nr):                       # nothing from row r + 1: exactly the row's own best, in its own columns
                assert lines[c.nc + r] == set(list(range(6))[:count] + list(range(64, 64 + max(0, count - 6)))), r
    if c.nr >= 64 and c.nc >= 64:
        assert st["rows_truncated"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.DIGIT_NAMES)
def test_digits_on_both_sides(K, handle, name):
    """5. a cut settled in each of the four passes, and keys that collapse to one float, on row samples and on column samples: every hub line is
    cut (truncated) and the host's decision on the candidates is exact"""
    c = C.case(name)
    db = handle(2)
    (criterion, count, filters), = c.runs
    lines, wide, st = check_call(K, db, c, upload(c.dense()), criterion, count, filters)
    assert st["rows_truncated"] >= len(C.HUB_ROWS) + len(C.HUB_COLS) and st["rows_refetched"] == 0
    for s in [c.nc + r for r in C.HUB_ROWS] + list(C.HUB_COLS):
        assert count <= len(lines[s]) < len(wide[s]), (name, s)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unrankable_row", "unrankable_col"])
def test_unrankable_cells(K, handle, name):
    """6. a k-mer count of 0 in the row array, and in the column array: every line with a cell the device cannot rank comes out whole, the others
    are cut"""
    c = C.case(name)
    db = handle(2)
    cells = upload(c.dense())
    for criterion, count, filters in c.runs:
        lines, wide, st = check_call(K, db, c, cells, criterion, count, filters)
        whole = C.unrankable_lines(c, criterion)
        zero = c.nc + 70 if name == "unrankable_row" else 70
        assert (zero in whole) == (criterion in ("min", "ani-shorter", "cosine")), criterion
        for s in range(c.nc + c.nr):
            if s in whole:
                assert lines[s] == wide[s], (criterion, s)
            elif len(wide[s]) > 20:
                assert len(lines[s]) < len(wide[s]), (criterion, s)


@pytest.mark.gpu
def test_refetch_on_both_sides(K, handle):
    """7. a bound inside the margin band leaves a truncated row line and a truncated column line short of `count` exact passes: both are fetched
    again whole, and the result is exact (the cell that completes either line lay below its cut)"""
    c = C.case("refetch")
    db = handle(2)
    (criterion, count, filters), = c.runs
    lines, wide, st = check_call(K, db, c, upload(c.dense()), criterion, count, filters)
    assert st["rows_refetched"] == 2 and st["triangle_reads"] >= 8
    for s in (c.nc + 10, 20):
        assert lines[s] == wide[s] and len(lines[s]) == 7
    cut = [s for s in range(c.nc + c.nr) if len(lines[s]) < len(wide[s])]
    assert len(cut) > 100


@pytest.mark.gpu
def test_offsets_beyond_32_bits(K, handle):
    """8. 65 600 x 65 600 cells (17.2 GB), zero but for a handful in the last two rows and the last two columns: r * nc + c in 64 bits"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 40 << 30:
        pytest.skip("needs 40 GB of free device memory, %.1f GB are free" % (free / 2 ** 30))
    c = C.case("big")
    cells = torch.zeros(C.BIG * C.BIG, dtype=torch.int32, device="cuda")
    r, x, v = c.triplets()
    cells[torch.from_numpy(r * C.BIG + x).cuda()] = torch.from_numpy(v.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    db = handle(2)
    for criterion, count, filters in c.runs:
        row_cand, col_cand = db.sampled_from_rect_device(cells.data_ptr(), c.nr, c.nc, criterion, count, c.a, c.b)
        want = C.expected_rect(K, c, criterion, count)
        got = K.sample_rows_select(criterion, count, C.K_LEN, c.kmers, [C.global_part(c.nr, c.nc, row_cand, col_cand)])
        assert got.nnz == sum(len(w) for w in want)
        for s in np.flatnonzero(np.diff(got.row_ptr.astype(np.int64))).tolist() + [0, c.nc - 1, c.nc + c.nr - 1]:
            assert list(zip(*(a.tolist() for a in got.row(s)))) == want[s], (count, s)
        if count == 8:
            assert row_cand.nnz == col_cand.nnz == len(c.cells) == 12
            assert row_cand.row(C.BIG - 1)[0].tolist() == [0, 33_000, 65_535, 65_536, C.BIG - 1] and col_cand.row(C.BIG - 1)[0].tolist() == [0, 40_000, C.BIG - 2, C.BIG - 1]
            assert row_cand.row(C.BIG - 1)[1].tolist() == [800, 50, 700, 650, 900]
        else:
            assert 2 <= len(row_cand.row(C.BIG - 1)[0]) < 5
    del cells


# ---- GPU: real cells ------------------------------------------------------------------------------------------------------------------------
def same_rows(x, y):
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in ("row_ptr", "col", "val"))


@pytest.mark.gpu
def test_db2db_sampled_on_a_real_cell(K, clade75, monkeypatch):
    """9. kmdb_db2db_sampled on two synth parts = kmdb_sampled_from_rect_device on the ORACLE's dense cell of the two, as uploaded; the same rows
    with KMDB_SP_ALL_TILES=1; only the touched tiles are read; the stats are filled"""
    monkeypatch.delenv("KMDB_SP_ALL_TILES", raising=False)
    c = clade75
    cells = upload(c.dense)
    tt = touched_tiles(c.dense)
    for criterion, count, filters in (("jaccard", 5, ()), ("mash-query", 3, ()), ("num-kmers", 3, (("jaccard", 0.3, None),))):
        rows, cols = c.drow.db2db_sampled(c.dcol, criterion, count, c.a, c.b, filters)
        st, ds = c.drow.db2db_sample_stats(), c.drow.db2db_stats()
        want_r, want_c = c.drow.sampled_from_rect_device(cells.data_ptr(), 150, 150, criterion, count, c.a, c.b, filters)
        assert same_rows(rows, want_r) and same_rows(cols, want_c), criterion
        assert ds["tiles"] == 9 and ds["tiles_touched"] == tt and 0 < tt < 9
        assert st["candidates"] == rows.nnz + cols.nnz > 0 and st["select_ms"] > 0 and st["triangle_reads"] >= 6 and st["d2h_bytes"] >= 8 * st["candidates"]
        assert st["rows_truncated"] > 0
        monkeypatch.setenv("KMDB_SP_ALL_TILES", "1")
        rows2, cols2 = c.drow.db2db_sampled(c.dcol, criterion, count, c.a, c.b, filters)
        assert same_rows(rows2, rows) and same_rows(cols2, cols) and c.drow.db2db_stats()["tiles_touched"] == 9
        monkeypatch.delenv("KMDB_SP_ALL_TILES")
    # the refusals of the dense call, under this entry's name; the handle still serves
    with pytest.raises(K.KmdbError, match="kmdb_db2db_sampled: sample_kmers is NULL"):
        c.drow.db2db_sampled(c.dcol, "jaccard", 5, c.a, None)
    assert c.drow.db2db_sampled(c.dcol, "jaccard", 5, c.a, c.b)[0].n_rows == 150


@pytest.fixture(scope="module")
def grid3(K, S, dev, tmp_path_factory):
    """CladeGenomes(90, 10, 1500, r1=0.75): three parts of 30 samples (ids 0, 3, ..; 1, 4, ..; 2, 5, ..: every clade in every part) and the whole
    collection in the order of the parts"""
    import torch
    device = torch.device("cuda", dev)
    tmp = tmp_path_factory.mktemp("grid3")
    g = S.CladeGenomes(90, 10, 1500, device=device, r1=0.75, r2=0.01, seed=23)
    ids = [list(range(p, 90, 3)) for p in range(3)]
    paths = [str(tmp / ("part%d.db" % p)) for p in range(3)] + [str(tmp / "whole.db")]
    for p, path in zip(ids + [ids[0] + ids[1] + ids[2]], paths):
        _synth_part(S, g, p, 18, path, device)
    hosts = [K.HostDB(p) for p in paths]
    dbs = [K.DeviceDB(h, device=dev, with_hashtables=True) for h in hosts]
    kmers = [h.sample_kmers.astype(np.uint32) + np.arange(h.N, dtype=np.uint32) * 37 % 500 for h in hosts[:3]]
    yield dict(parts=dbs[:3], whole=dbs[3], kmers=kmers, all_kmers=np.concatenate(kmers), k=18)
    for d in dbs:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("criterion,count,filters", [("jaccard", 5, ()), ("mash-query", 3, ()), ("num-kmers", 3, (("jaccard", 0.2, None),))])
def test_a_grid_of_three_parts(K, grid3, criterion, count, filters):
    """10. the candidates of the three off-diagonal cells and the three diagonal all2all_sampled results, merged by the host = all2all_sampled on
    the whole collection"""
    g = grid3
    n, N = 30, 90
    want = g["whole"].all2all_sampled(criterion, count, g["all_kmers"], filters)

    def lift(sp, first, shift):
        """rows of a cell's output as a part of the collection: its rows from `first` on, its ids shifted"""
        ptr = np.zeros(N + 1, np.uint64)
        ptr[first + 1:first + n + 1] = sp.row_ptr[1:]
        ptr[first + n + 1:] = sp.row_ptr[-1]
        return ptr, (sp.col + np.uint32(shift)).astype(np.uint32), sp.val.astype(np.uint32)

    parts = []
    for i in range(3):
        parts.append(lift(g["parts"][i].all2all_sampled(criterion, count, g["kmers"][i], filters), i * n, i * n))
        for j in range(i):
            rows, cols = g["parts"][i].db2db_sampled(g["parts"][j], criterion, count, g["kmers"][i], g["kmers"][j], filters)
            assert rows.nnz and cols.nnz
            parts += [lift(rows, i * n, j * n), lift(cols, j * n, i * n)]
    got = K.sample_rows_select(criterion, count, g["k"], g["all_kmers"], parts, filters)
    assert rows_of(got) == rows_of(want) and want.nnz > N


# ---- GPU: the front-end ---------------------------------------------------------------------------------------------------------------------
def _cli(*args, env=None):
    exe = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=dict(os.environ, KMDB_VERBOSE="1", **(env or {})))
    assert r.returncode == 0, r.stderr
    return r


def file_rows(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[1].startswith(b"query-samples,total-kmers,") and lines[-1] == b""
    return [[(int(cv.split(b":")[0]) - 1, int(cv.split(b":")[1])) for cv in ln.split(b",")[2:-1]] for ln in lines[2:-1]]


@pytest.mark.gpu
@pytest.mark.parametrize("tag,opts", [("sr_jaccard5", ["-sample-rows", "jaccard:5"]), ("sr_numkmers3_min", ["-sample-rows", "num-kmers:3", "-min", "jaccard:0.02"])])
def test_front_end_selects_on_the_device(K, golden_dir, dev, tmp_path, tag, opts):
    """11. all2all-parts over the two virus parts writes the rows of the reference's golden; the same bytes with -gpus 2 and with
    KMDB_PARTS_HOST_SAMPLER=1; the per-cell line of KMDB_VERBOSE appears on the device path only"""
    t = lambda n: str(tmp_path / n)             # noqa: E731
    with open(t("db.list"), "w") as f:
        f.write(os.path.join(golden_dir, "virus_k18_part1.db") + "\n" + os.path.join(golden_dir, "virus_k18_part2.db") + "\n")
    r = _cli("all2all-parts", *opts, t("db.list"), t("dev.csv"))
    assert file_rows(t("dev.csv")) == golden_rows(golden_dir, "virus_k18", tag)
    assert r.stderr.count(LINE) == 1 and "(2,1)" in [ln for ln in r.stderr.split("\n") if LINE in ln][0]
    r2 = _cli("all2all-parts", *opts, "-gpus", "2", t("db.list"), t("g2.csv"))
    assert r2.stderr.count(LINE) == 1
    r3 = _cli("all2all-parts", *opts, t("db.list"), t("host.csv"), env={"KMDB_PARTS_HOST_SAMPLER": "1"})
    assert LINE not in r3.stderr
    dev_bytes = open(t("dev.csv"), "rb").read()
    assert open(t("g2.csv"), "rb").read() == dev_bytes and open(t("host.csv"), "rb").read() == dev_bytes


@pytest.mark.gpu
def test_front_end_keeps_the_host_path_where_it_must(K, golden_dir, dev, tmp_path):
    """11. the random strategy, 13 bounds and KMDB_PARTS_DENSE_CELLS=1 still succeed, on the host: no per-cell line; 13 bounds that keep
    everything and dense cells write the bytes of the device path"""
    t = lambda n: str(tmp_path / n)             # noqa: E731
    with open(t("db.list"), "w") as f:
        f.write(os.path.join(golden_dir, "virus_k18_part1.db") + "\n" + os.path.join(golden_dir, "virus_k18_part2.db") + "\n")
    r = _cli("all2all-parts", "-sample-rows", "3", t("db.list"), t("random.csv"))
    assert LINE not in r.stderr and all(len(row) <= 3 for row in file_rows(t("random.csv")))
    bounds = []
    for m in ("jaccard", "min", "max", "cosine", "ani", "ani-shorter"):
        bounds += ["-min", m + ":-1e9", "-max", m + ":1e9"]
    bounds += ["-min", "num-kmers:1"]
    r = _cli("all2all-parts", "-sample-rows", "jaccard:5", *bounds, t("db.list"), t("b13.csv"))
    assert LINE not in r.stderr
    r = _cli("all2all-parts", "-sample-rows", "jaccard:5", t("db.list"), t("dense.csv"), env={"KMDB_PARTS_DENSE_CELLS": "1"})
    assert LINE not in r.stderr
    want = golden_rows(golden_dir, "virus_k18", "sr_jaccard5")
    assert file_rows(t("b13.csv")) == want and file_rows(t("dense.csv")) == want
