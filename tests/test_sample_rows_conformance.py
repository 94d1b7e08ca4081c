"""csrc/sample_rows.hip at its edges: the radix select (sr_tile_kernel / sr_select_kernel) and the row sort (sr_sort_rows_kernel) on the crafted
matrices of sample_rows_cases.py, through kmdb_sampled_from_dense_device.  Every GPU assertion compares with the python restatement of the
sampler over the whole matrix (expected_rows) or with the bracket derived from the kernel's constants (sample_rows_cases.BAND_LO / BAND_HI),
never with another device result — but for "the parts merged = the one call" of the flat ranges, which is compared with expected_rows too."""
import numpy as np
import pytest

import sample_rows_cases as C
from sample_rows_cases import full_part, rows_of
from test_sample_rows_device import S, dev, expected_rows, synth150, synth_expected  # noqa: F401  (S, dev, synth150: fixtures)

LOG_CRITERIA = ("mash", "ani", "ani-shorter", "mash-query")


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_hold_what_they_are_named_for():
    """the key restatement's digit assertions for every digit case, the float collapses, the row lengths, the unrankable rows, and a bracket
    that is not vacuous"""
    C.census_digits()
    C.census_collapse()
    C.census_bracket()
    C.census_rowlen()
    C.census_unrankable()


@pytest.mark.parametrize("name", C.NAMES)
def test_host_select_on_the_whole_matrix(K, name):
    """kmdbh_sample_rows_select over the whole crafted matrix as one part = the python restatement, the unrankable cells included: pins the
    restatement and the host's decision (NaN scores last) on the very inputs the device is judged by"""
    c = C.CASES[name]
    part = full_part(c.tri, c.N)
    for criterion, count in c.runs:
        assert rows_of(K.sample_rows_select(criterion, count, C.K_LEN, c.kmers, [part])) == C.expected(K, name, criterion, count), (criterion, count)


def test_an_unrankable_cell_needs_its_whole_row(K):
    """why a row with an unrankable cell comes out whole: rank that cell above every number, cut hub 63's row at count = 2 — {the unrankable
    cell, the best finite one} — and the host, which scores the cell NaN under the four log measures, no longer finds the row's two best"""
    c = C.CASES["unrankable"]
    ptr, col, val = full_part(c.tri, c.N)
    for criterion in C.CRITERIA:
        sp, _, _, p = C.sym_rows("unrankable", criterion)
        a, b = int(sp[63]), int(sp[64])
        bad = ~np.isfinite(p[a:b])
        if not bad.any():
            continue
        assert np.count_nonzero(bad) == 1 and b - a == 5
        keep = np.ones(len(col), bool)
        keep[a:b] = bad | (p[a:b] == p[a:b][~bad].max())
        cut = ptr.copy()
        cut[64:] -= np.uint64(3)
        got = rows_of(K.sample_rows_select(criterion, 2, C.K_LEN, c.kmers, [(cut, col[keep], val[keep])]))
        assert (got[63] != C.expected(K, "unrankable", criterion, 2)[63]) == (criterion in LOG_CRITERIA), criterion


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(K, S, dev):
    """kmdb_sampled_from_dense_device needs only the handle's N: a view of N samples with the empty pattern alone (N singleton patterns where
    the upload refuses that)"""
    import torch
    made = {}

    def get(N):
        if N in made:
            return made[N]
        z = lambda n: torch.zeros(n, dtype=torch.int64)     # noqa: E731
        one = torch.ones(N, dtype=torch.int64)
        pats = [{"num_kmers": z(1), "parent": torch.tensor([-1]), "num_samples": z(1), "num_local": z(1), "local_ptr": z(2), "local_ids": z(0)},
                {"num_kmers": torch.cat([z(1), one]), "parent": -torch.ones(N + 1, dtype=torch.int64), "num_samples": torch.cat([z(1), one]),
                 "num_local": torch.cat([z(1), one]), "local_ptr": torch.cat([z(1), torch.arange(N + 1)]), "local_ids": torch.arange(N)}]
        for n, pat in enumerate(pats):
            arr = S.to_view_arrays(pat)
            view = K.make_view(C.K_LEN, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                               arr["data_offset"], arr["data"])
            try:
                made[N] = K.DeviceDB(view, device=dev)
                return made[N]
            except K.KmdbError:
                if n:
                    raise

    yield get
    for db in made.values():
        db.close()


def upload(tri):
    import torch
    return torch.from_numpy(tri.view(np.int32)).cuda()         # (cells >= 2^31 go in as their bits)


def check_candidates(c, name, criterion, count, cand):
    """2. ascending distinct columns, val = the crafted cell; 3. a truncated row brackets its candidates from both sides; 4. a row with fewer
    than `count` cells, or with a cell the device cannot rank, comes out whole"""
    rows, _ = C.row_models(name, criterion, count)
    assert cand.measure is None and cand.n_rows == c.N
    for s, model in enumerate(rows):
        cols, vals = cand.row(s)
        cols = cols.astype(np.int64)
        assert (np.diff(cols) > 0).all(), (name, criterion, count, s)
        hi, lo = np.maximum(cols, s), np.minimum(cols, s)
        assert np.array_equal(vals, c.tri[hi * (hi - 1) // 2 + lo]), (name, criterion, count, s)
        if model[0] == "whole":
            assert np.array_equal(cols, model[1]), (name, criterion, count, s)
        else:
            assert np.isin(model[1], cols).all() and np.isin(cols, model[2]).all(), (name, criterion, count, s, len(model[1]), len(cols), len(model[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.NAMES)
def test_crafted_matrix(K, handle, name):
    """every (criterion, count) of a case: 1. the rows the host selects from the device's candidates = expected_rows, exactly; 2. - 4. the
    candidates (check_candidates); 5. rows_truncated = the model's count of rows cut with something left below the cut; 6. no row fetched again"""
    c = C.CASES[name]
    db = handle(c.N)
    cells = upload(c.tri)
    for criterion, count in c.runs:
        cand = db.sampled_from_dense_device(cells.data_ptr(), criterion, count, c.kmers)
        st = db.sample_stats()
        got = K.sample_rows_select(criterion, count, C.K_LEN, c.kmers, [cand])
        assert rows_of(got) == C.expected(K, name, criterion, count), (criterion, count)
        check_candidates(c, name, criterion, count, cand)
        assert st["rows_truncated"] == C.row_models(name, criterion, count)[1], (criterion, count)
        assert st["rows_refetched"] == 0 and st["candidates"] == cand.nnz


@pytest.mark.gpu
def test_flat_ranges_of_the_crafted_matrix(K, handle):
    """the rowlen matrix in nine ranges that cover its triangle (sample_rows_cases.RANGE_CUTS): a range of whole rows, one cell, a range inside
    one hub's triangle row, a start mid-row inside a diagonal tile, an end at the last cell; the candidates of the parts, merged by the host,
    give the rows of the one call and of expected_rows"""
    c = C.CASES["rowlen"]
    db = handle(c.N)
    cells = upload(c.tri)
    cuts = C.RANGE_CUTS
    for criterion, count in (("num-kmers", 512), ("jaccard", 512), ("num-kmers", 32)):
        parts = [db.sampled_from_dense_device(cells.data_ptr() + 4 * lo, criterion, count, c.kmers, cell_lo=lo, cell_hi=hi) for lo, hi in zip(cuts, cuts[1:])]
        for p, lo, hi in zip(parts, cuts, cuts[1:]):
            row = np.repeat(np.arange(c.N), np.diff(p.row_ptr).astype(np.int64))
            col = p.col.astype(np.int64)
            x = np.maximum(row, col) * (np.maximum(row, col) - 1) // 2 + np.minimum(row, col)
            assert ((x >= lo) & (x < hi)).all() and np.array_equal(p.val, c.tri[x]) and (np.diff(col)[np.diff(row) == 0] > 0).all()
        one_cell = parts[cuts.index(C.flat(1500, 7))]
        assert (one_cell.nnz, one_cell.row(1500)[0].tolist(), one_cell.row(7)[0].tolist()) == (2, [7], [1500])
        want = C.expected(K, "rowlen", criterion, count)
        assert rows_of(K.sample_rows_select(criterion, count, C.K_LEN, c.kmers, parts)) == want
        whole = db.sampled_from_dense_device(cells.data_ptr(), criterion, count, c.kmers)
        assert rows_of(K.sample_rows_select(criterion, count, C.K_LEN, c.kmers, [whole])) == want


@pytest.fixture(scope="module")
def sparse301(K, O, S, tmp_path_factory):
    """the collection of test_sample_rows_device.test_mostly_untouched_tiles: clades of 6 from independent roots, most tiles never touched"""
    N, k = 301, 25
    g, pat = S.synth_database(N, 6, 3000, k=k, seed=41, r1=0.75)
    arr = S.to_view_arrays(pat)
    path = str(tmp_path_factory.mktemp("sr") / "sparse.db")
    S.write_db(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr)
    tri = O.OracleDB(path, skip_hashtables=True).all2all_dense().copy()
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"])
    return dict(N=N, k=k, tri=tri, kmers=np.asarray(pat["sample_counts"], dtype=np.int64), view=view, expected={})


@pytest.mark.gpu
@pytest.mark.parametrize("width", [32, 50])
def test_tile_flags_at_other_widths(K, dev, synth150, sparse301, monkeypatch, width):
    """all2all_sampled on fresh handles under KMDB_BLOCK_WIDTH = 32 and 50: the tile flags of the block-record pipeline at a width that is not
    64 — SrJob.W and the `lane < W` guards of sr_tile_kernel — on a full and on a mostly untouched matrix"""
    monkeypatch.delenv("KMDB_SP_ALL_TILES", raising=False)
    monkeypatch.setenv("KMDB_BLOCK_WIDTH", str(width))
    for d, runs in ((synth150, (("jaccard", 5), ("mash-query", 20), ("num-kmers", 1))), (sparse301, (("jaccard", 3), ("mash", 8), ("num-kmers", 5)))):
        db = K.DeviceDB(d["view"], device=dev)
        for criterion, count in runs:
            got = db.all2all_sampled(criterion, count, d["kmers"])
            assert db.stats()["path"] == K.capi.PATH_RECORDS, (d["N"], criterion)
            assert rows_of(got) == synth_expected(K, d, criterion, count), (d["N"], criterion, count)
            assert db.sample_stats()["rows_refetched"] == 0
        db.close()
