"""db2db conformance: the branches of csrc/db2db.hip (all2all-parts' cell of two databases) that no other test reaches, each with a case
of tests/db2db_cases.py built around the engine's own thresholds, and a census on the host that proves what the cases hold before a
device runs.

  1. pair counts of two digits: d2_emit_kernel writes one block record per base-2^dbits digit of a pair's count (nd, the j loop,
     digit | j << dbits) and wide_weight (a2a_blocks.hip) shifts it back.  S (dbits 17, list store) and C (dbits 16, root-path climb) hold
     pairs that share 2^dbits - 1, 2^dbits (a weight-0 record), 2^dbits + 1, ... k-mers.
  2. the counted second attempt of the record pool: P yields 1.36 x the slots of the first pool; KMDB_VERBOSE's lines are the witness.
  3. key widths: K1 / K2 have pattern counts of 2^n and 2^n - 1 (and of 2), the last DFS nodes of both sides share k-mers.
  4. the sort inside kmdb_rect_sort_apply: E2047 / E2048 (one-pass counting sort) and E2050 (radix sort) block pairs.
  5. a part against itself with several blocks: Zself; and the degenerate cells Z0 (nothing shared), Z1 / Z2 (a part of one sample).

The reference is the CPU oracle's db2db (the C restatement, pinned to the reference's goldens in test_oracle_golden.py) wherever its
cost — |row list| x |column list| additions per shared k-mer — stays small, and the definition in numpy (db2db_cases.Case.definition)
for P; test_references_agree holds the two against each other on every case the oracle can afford.  All comparisons are exact.

Out of reach, on purpose: counts of three and four digits through db2db need dbits <= 10 with counts >= 2^20, cells of 8 GB and more;
the shifts of wide_weight for j >= 2 are shared with all2all, where test_few_streams_record_forms goes up to four digits, and db2db's
own code is the generic j loop that two digits exercise.  The refusals "more than 2^22 block pairs" and "do not fit the LDS" come after
dense allocations of tens of GB; the scalar branch of kmdb_probe needs tables of a capacity below 4 or at an odd offset, which the
fabricated tables of test_new2all_conformance.py hold (test_probe_tables_through_db2db runs them through this path)."""
import os
import re

import numpy as np
import pytest

import db2db_cases as D
from test_gpu_parity import _Laps
from test_kernel_variants import _S

CELLS = ("S", "C", "K1", "K2", "E2047", "E2048", "E2050", "P", "Z0", "Z1", "Z2")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


@pytest.fixture
def env(monkeypatch):
    """the switches db2db reads (at every call), all unset; the monkeypatch that sets one for the test"""
    for name in ("KMDB_D2_NO_STORE", "KMDB_SP_ALL_TILES", "KMDB_VERBOSE"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


class _Lap(_Laps):
    """the laps of _Laps, printed as well (pytest -s / the captured output of a failing test)"""

    def done(self):
        print(self.name + " " + " ".join(self.laps), flush=True)
        super().done()


class _Built:
    """a case as two .db files; the expectation is computed once, shared by the tests that need it, never written to"""

    def __init__(self, case, folder):
        import time
        t = time.time()
        self.case = case
        S = _S()
        case.row.write(S, os.path.join(folder, case.name + "_rows.db"))
        if case.col is not case.row:
            case.col.write(S, os.path.join(folder, case.name + "_cols.db"))
        self.seconds = time.time() - t
        self._exp = None

    def affordable(self):
        return self.case.census()["oracle_cost"] <= D.ORACLE_BUDGET

    def oracle(self, O):
        orow = O.OracleDB(self.case.row.path)
        ocol = orow if self.case.col is self.case.row else O.OracleDB(self.case.col.path)
        try:
            return orow.db2db(ocol)
        finally:
            orow.close()
            ocol.close()

    def expected(self, O):
        if self._exp is None:
            self._exp = self.oracle(O) if self.affordable() else self.case.definition()
            self._exp.setflags(write=False)
            self._expT = np.ascontiguousarray(self._exp.T)
            self._expT.setflags(write=False)
        return self._exp, self._expT

    def handles(self, K, dev):
        row = K.DeviceDB(K.HostDB(self.case.row.path), device=dev, with_hashtables=True)
        if self.case.col is self.case.row:
            return row, row
        try:
            return row, K.DeviceDB(K.HostDB(self.case.col.path), device=dev, with_hashtables=True)
        except Exception:
            row.close()
            raise


@pytest.fixture(scope="module")
def built(K, tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("db2db"))
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Built(D.case(name), folder)
        return made[name]
    return get


def _same(got, exp, what):
    """exact equality of a cell; a failure names the number of differing cells and the first three with both values (an error that is a
    multiple of 2^dbits is the digit index j of d2_emit_kernel / wide_weight)"""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if np.array_equal(got, exp):
        return
    bad = np.argwhere(got != exp)
    first = ["(%d, %d) got %d, expected %d" % (r, c, int(got[r, c]), int(exp[r, c])) for r, c in bad[:3].tolist()]
    pytest.fail("%s: %d of %d cells differ; first: %s" % (what, bad.shape[0], exp.size, "; ".join(first)))


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
def test_references_agree(O, built):
    """the definition in numpy == the CPU oracle on S, C, K, E, Z and the scaled-down copy of P (every case the oracle can afford: P itself
    is beyond the budget); on the small cases the definition written over the non-zeros == the product of the dense matrices.  The
    seconds of building each case's two .db files are printed (pytest -s)."""
    pinned = []
    for name in D.NAMES:
        b = built(name)
        print("%s: databases in %.1f s, oracle cost %d" % (name, b.seconds, b.case.census()["oracle_cost"]))
        if not b.affordable():
            continue
        pinned.append(name)
        got, want = b.oracle(O), b.case.definition()
        _same(got, want, "oracle against the definition, case " + name)
        if b.case.row.P * b.case.col.P * b.case.col.N <= 1 << 27:
            assert np.array_equal(b.case.dense_product(), want), name
    assert pinned == [n for n in D.NAMES if n != "P"]
    assert all(built(n).case.definition().any() for n in D.NAMES if n != "Z0") and not built("Z0").case.definition().any()


def test_cases_hold_what_the_gpu_tests_rely_on():
    """The census.  Geometry as the engine computes it (db2db_cases.geometry restates db2db.hip:499-501, engine_constants() checks that
    the source still says so).  S, C: the heavy pairs read back from the dictionaries are the planned ones; 2^dbits - 1 has one digit,
    every count from 2^dbits on exactly two; 2^dbits has low digit 0; counts with both digits non-zero exist; S is at the list store's
    limit, C beyond it with partial last blocks; heavy lists over two blocks, inside the last block, up to the last sample id; a light
    pattern inherits a heavy one's ids.  K: pattern counts 2^n / 2^n - 1 / 2, the last and first DFS nodes share k-mers, the largest key
    is not the "no hit" key.  E: 2047 <= CS_MAX_KEYS == 2048 < 2050 block pairs, all of them hit in E2048, empty block rows and columns
    next to hit ones in the others.  P: every paired pattern covers every block, the records exceed the first pool by POOL_FACTOR."""
    k = D.engine_constants()
    assert k == {"CS_MAX_KEYS": 2048, "D2_GRAB": 512, "D2_CURSORS": 256, "D2_SETS_MAX_NB": 64}, k      # a2a_blocks.hip:2222, db2db.hip:184, :132
    for name, nbs, key_bits, dbits in (("S", (64, 64), 13, 17), ("C", (129, 65), 14, 16)):
        c = D.case(name)
        g = c.geo
        assert (g["nbr"], g["nbc"], g["key_bits"], g["dbits"]) == nbs + (key_bits, dbits), (name, g)
        assert D.geometry(c.col.N, c.row.N)["dbits"] == dbits                  # (the other direction)
        pr, pc, n = c.pairs()
        found = {(a, b): x for a, b, x in zip(pr.tolist(), pc.tolist(), n.tolist())}
        assert all(found[(a, b)] == x for a, b, x in c.planned) and len(found) == len(c.planned), name
        heavy = [x for _, _, x in c.about["heavy"]]
        b = 1 << dbits
        assert {b - 1, b, b + 1} <= set(heavy) and c.census()["largest"] == max(heavy) < b * b, (name, heavy)
        assert all(len(D.digits(x, dbits)) == (2 if x >= b else 1) for x in heavy), (name, heavy)
        assert D.digits(b, dbits) == [0, 1] and D.digits(b - 1, dbits) == [b - 1]
        assert sum(all(D.digits(x, dbits)) and x >= b for x in heavy) >= 2, (name, heavy)             # both digits non-zero
        assert all(x < 1 << 3 for a, bb, x in c.planned if (a, bb, x) not in c.about["heavy"])        # everything else is light
        full_r, full_c = c.row.full(), c.col.full()
        lists = [full_r[p] for p in c.about["heavy_rows"]] + [full_c[p] for p in c.about["heavy_cols"]]
        assert all(2 <= f.size <= 4 for f in lists), name
        assert any(D.n_blocks_of(f) == 2 and f[-1] // 64 == f[0] // 64 + 1 for f in lists)            # across a block boundary
        assert name != "S" or any(f[0] // 64 == (c.row.N - 1) // 64 for f in lists[:4])              # S: inside the last block, a full one
        assert any(f[-1] == c.row.N - 1 for f in lists[:4]) and any(f[-1] == c.col.N - 1 for f in lists[4:])  # the last sample ids
        desc = c.about["descendant"]
        anc = c.about["heavy_rows"][0 if name == "S" else 2]
        assert int(c.row.pat["parent"][desc]) == anc and np.array_equal(full_r[desc][: full_r[anc].size], full_r[anc])
        assert any(a == desc for a, _, _ in c.planned)
        assert sum(a == c.about["heavy_rows"][0] for a, _, _ in c.planned) >= 3                        # one row list, pairs of one and of two digits
        assert c.census()["records"] + 6 * len(found) < D.first_pool_slots(len(found), c.row.N, c.col.N)      # (the first pool holds them)
    s, c = D.case("S"), D.case("C")
    assert s.geo["nbr"] == s.geo["nbc"] == k["D2_SETS_MAX_NB"] and s.row.N % 64 == 0                   # at the store's limit, no partial block
    assert min(c.geo["nbr"], c.geo["nbc"]) > k["D2_SETS_MAX_NB"] and c.row.N % 64 == 63 and c.col.N % 64 == 63
    assert s.geo["n_states"] > k["CS_MAX_KEYS"] and c.geo["n_states"] > k["CS_MAX_KEYS"]              # both on the radix sort
    # K
    for name, Pr, Pc, widths in (("K1", 512, 511, (10, 9)), ("K2", 2, 256, (2, 9))):
        c = D.case(name)
        assert (c.row.P, c.col.P) == (Pr, Pc) and D.key_widths(Pr, Pc) == widths and max(c.row.N, c.col.N) <= 300
        dr, dc = D.dfs_index(c.row.pat), D.dfs_index(c.col.pat)
        pr, pc, _ = c.pairs()
        keys = set(zip(dr[pr].tolist(), dc[pc].tolist()))
        assert {(Pr - 1, Pc - 1), (1, Pc - 1), (Pr - 1, 1), (1, 1)} <= keys, name
        rbits, cbits = widths
        assert ((Pr - 1) << cbits | (Pc - 1)) < (1 << (rbits + cbits)) - 1
        assert sorted(dr.tolist()) == list(range(Pr)) and (name == "K2" or (dr != np.arange(Pr)).any())      # (the DFS order is not the pid order)
    # E
    e = {n: D.case(n) for n in ("E2047", "E2048", "E2050")}
    assert [(x.geo["nbr"], x.geo["nbc"]) for x in e.values()] == [(23, 89), (32, 64), (41, 50)]
    assert e["E2047"].geo["n_states"] == k["CS_MAX_KEYS"] - 1 and e["E2048"].geo["n_states"] == k["CS_MAX_KEYS"] and e["E2050"].geo["n_states"] == k["CS_MAX_KEYS"] + 2
    assert e["E2048"].census()["streams"].all()
    for n in ("E2047", "E2050"):
        hit = e[n].census()["streams"]
        for axis in (0, 1):
            assert 0 < int(hit.any(axis=axis).sum()) < hit.shape[1 - axis], n                         # whole block columns / rows stay empty
    assert all(x.census()["largest"] <= 5 and x.row.N % 64 and x.col.N % 64 for x in e.values())
    # P and its small copy
    for name in ("P", "Ps"):
        c = D.case(name)
        pr, pc, _ = c.pairs()
        assert len(c.row.full()) < 100 and len(c.col.full()) < 100 and pr.size == 3000
        assert all(D.n_blocks_of(c.row.full()[p]) == c.geo["nbr"] for p in np.unique(pr)) and all(D.n_blocks_of(c.col.full()[p]) == c.geo["nbc"] for p in np.unique(pc))
        assert c.census()["records"] == 3000 * c.geo["n_states"] and c.census()["largest"] <= 3
    p = D.case("P")
    assert (p.row.N, p.col.N) == (D.case("C").row.N, D.case("C").col.N)                              # C's geometry
    assert p.census()["records"] >= D.POOL_FACTOR * D.first_pool_slots(3000, p.row.N, p.col.N), (p.census()["records"], D.first_pool_slots(3000, p.row.N, p.col.N))
    assert (D.case("Ps").row.N, D.case("Ps").col.N) == (520, 260)
    # Z
    z0, z1, z2, zs = (D.case(n) for n in ("Z0", "Z1", "Z2", "Zself"))
    assert z0.pairs()[0].size == 0 and z0.row.kmers.size and z0.col.kmers.size
    assert z1.col.N == 1 and (z2.row.N, z2.col.N) == (65, 1) and z2.definition()[64, 0] > 0 and z1.definition().any()
    assert zs.row is zs.col and zs.row.N == 300 and zs.geo["nbr"] == 5


# ------------------------------------------------------------------------------------------------------------------------------------
# on the device
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CELLS)
def test_dense_cell(K, O, dev, env, built, name):
    """kmdb_db2db_dense, rows x columns == the expectation and columns x rows == its transpose.  The list store shows in device_bytes: S's
    handles grow by it, C's (parts beyond 4096 samples) and P's do not."""
    lap = _Lap("db2db dense " + name)
    b = built(name)
    exp, expT = b.expected(O)
    lap("databases, expectation")
    a, c = b.handles(K, dev)
    try:
        before = a.stats()["device_bytes"], c.stats()["device_bytes"]
        _same(a.db2db(c), exp, "case %s, rows x columns" % name)
        _same(c.db2db(a), expT, "case %s, columns x rows" % name)
        after = a.stats()["device_bytes"], c.stats()["device_bytes"]
        if name == "S":
            assert after[0] == before[0] + b.case.row.P * 64 * 8 and after[1] == before[1] + b.case.col.P * 64 * 8, (before, after)
        elif name in ("C", "P"):
            assert after == before, (before, after)
        lap("both directions")
    finally:
        a.close()
        c.close()
    lap.done()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CELLS)
def test_sparse_cell(K, O, dev, env, built, name):
    """kmdb_db2db_sparse_filtered without filters: the CSR of the expectation's non-zeros (row pointers, ascending columns, values), both
    ways round; tiles_touched == the 64 x 64 tiles of the expectation that hold a non-zero (a weight-0 record of a count of 2^dbits
    flags a tile that its high digit fills); with KMDB_SP_ALL_TILES=1 (every tile scanned) the same rows."""
    lap = _Lap("db2db sparse " + name)
    b = built(name)
    exp, expT = b.expected(O)
    a, c = b.handles(K, dev)
    try:
        for r, q, e, what in ((a, c, exp, "rows x columns"), (c, a, expT, "columns x rows")):
            rp, col, val = D.csr_of(e)
            for all_tiles in (False, True):
                if all_tiles:
                    env.setenv("KMDB_SP_ALL_TILES", "1")
                else:
                    env.delenv("KMDB_SP_ALL_TILES", raising=False)
                sp = r.db2db_sparse(q)
                st = r.db2db_stats()
                assert sp.n_rows == e.shape[0] and np.array_equal(sp.row_ptr, rp), (name, what, all_tiles, "row_ptr")
                assert np.array_equal(sp.col, col) and np.array_equal(sp.val, val), (name, what, all_tiles, "columns / values")
                tiles = ((e.shape[0] + 63) // 64) * ((e.shape[1] + 63) // 64)
                assert st["tiles"] == tiles and st["tiles_touched"] == (tiles if all_tiles else D.tiles_of(e)), (name, what, all_tiles, st)
            lap(what)
    finally:
        a.close()
        c.close()
    lap.done()


@pytest.mark.gpu
def test_two_digit_records_from_the_climbing_kernel_at_a_store_capable_size(K, O, dev, env, built):
    """S with KMDB_D2_NO_STORE=1 on fresh handles: d2_emit_kernel<*, false> (the root-path climb) at 4096 samples — the same cell,
    device_bytes unchanged by the call.  (test_dense_cell[S] shows the growth without the variable: the store was used there.)"""
    b = built("S")
    exp, expT = b.expected(O)
    env.setenv("KMDB_D2_NO_STORE", "1")
    a, c = b.handles(K, dev)
    try:
        before = a.stats()["device_bytes"], c.stats()["device_bytes"]
        _same(a.db2db(c), exp, "case S without the store, rows x columns")
        _same(c.db2db(a), expT, "case S without the store, columns x rows")
        assert (a.stats()["device_bytes"], c.stats()["device_bytes"]) == before
    finally:
        a.close()
        c.close()


@pytest.mark.gpu
def test_second_call_with_the_store_in_place(K, O, dev, env, built):
    """S twice on one pair of handles, dense and sparse: the second call finds the list stores made by the first (device_bytes grows once)
    and sizes a fresh pool; the same cell"""
    b = built("S")
    exp, expT = b.expected(O)
    a, c = b.handles(K, dev)
    try:
        _same(a.db2db(c), exp, "case S, first call")
        grown = a.stats()["device_bytes"], c.stats()["device_bytes"]
        _same(a.db2db(c), exp, "case S, second call")
        _same(c.db2db(a), expT, "case S, columns x rows on the rows' stores")
        sp = a.db2db_sparse(c)
        rp, col, val = D.csr_of(exp)
        assert np.array_equal(sp.row_ptr, rp) and np.array_equal(sp.col, col) and np.array_equal(sp.val, val)
        assert (a.stats()["device_bytes"], c.stats()["device_bytes"]) == grown
    finally:
        a.close()
        c.close()


POOL_LINE = re.compile(r"\[kmdb\] db2db: (\d+) pattern pairs, pool for (\d+) records \((estimate|counted)\)(: too small)?")


@pytest.mark.gpu
def test_counted_pool(K, O, dev, env, built, capfd):
    """P: the first pool (six records per pair, a floor of 130 grabs per cursor) overflows, d2_emit_kernel<true, *> counts, and the pool made to
    measure takes the records.  KMDB_VERBOSE's lines (the library's stderr) are the witness: "(estimate): too small", then "(counted)" with
    the census of db2db_cases — in both directions and again on a second call with the same handles; every cell == the definition."""
    lap = _Lap("db2db counted pool")
    b = built("P")
    exp, expT = b.expected(O)
    assert not b.affordable()                                   # (the numpy definition is this case's reference)
    records = b.case.census()["records"]
    lap("databases, definition")
    a, c = b.handles(K, dev)
    try:
        env.setenv("KMDB_VERBOSE", "1")
        for r, q, e, what in ((a, c, exp, "rows x columns"), (c, a, expT, "columns x rows"), (a, c, exp, "rows x columns, second call")):
            capfd.readouterr()
            got = r.db2db(q)
            err = capfd.readouterr().err
            lines = [(int(m.group(1)), int(m.group(2)), m.group(3), m.group(4) is not None) for m in POOL_LINE.finditer(err)]
            assert lines == [(3000, 6 * 3000, "estimate", True), (3000, records, "counted", False)], (what, lines, err[-2000:])
            _same(got, e, "case P, " + what)
            lap(what)
    finally:
        a.close()
        c.close()
    lap.done()


@pytest.mark.gpu
def test_degenerate_cells(K, O, dev, env, built):
    """Z0: nothing shared (the run of slots without a hit is no pattern pair: nruns == 0) — a zero cell, an empty CSR with row_ptr all 0, no
    tile touched, no list store made.  Z1, Z2: a part of ONE sample gives cells of
    (nr, 1) and (1, nc).  Zself: a part of 300 samples (5 blocks) against itself, one handle on both sides: symmetric, the samples' k-mer
    counts on the diagonal, == the expectation; its CSR."""
    b = built("Z0")
    a, c = b.handles(K, dev)
    try:
        before = a.stats()["device_bytes"], c.stats()["device_bytes"]
        for r, q in ((a, c), (c, a)):
            got = r.db2db(q)
            assert got.shape == (r.N, q.N) and not got.any()
            assert (a.stats()["device_bytes"], c.stats()["device_bytes"]) == before      # no pair: the call ends before list stores and pool
            sp = r.db2db_sparse(q)
            assert sp.n_rows == r.N and sp.nnz == 0 and sp.col.size == 0 and not sp.row_ptr.any() and sp.row_ptr.size == r.N + 1
            assert r.db2db_stats()["tiles_touched"] == 0 and r.db2db_stats()["tiles"] == 4
    finally:
        a.close()
        c.close()
    for name in ("Z1", "Z2"):
        b = built(name)
        exp, expT = b.expected(O)
        a, c = b.handles(K, dev)
        try:
            got, gotT = a.db2db(c), c.db2db(a)
            assert got.shape == (b.case.row.N, 1) and gotT.shape == (1, b.case.row.N) and got.any()
            _same(got, exp, name)
            _same(gotT, expT, name + " transposed")
        finally:
            a.close()
            c.close()
    b = built("Zself")
    exp, _ = b.expected(O)
    part = b.case.row
    counts = np.zeros(part.N, dtype=np.int64)                   # k-mers of a sample: those of every pattern that lists it
    for p, full in enumerate(part.full()):
        counts[full] += int(part.pat["num_kmers"][p])
    d, same = b.handles(K, dev)
    assert same is d
    try:
        got = d.db2db(d)
        _same(got, exp, "Zself")
        assert np.array_equal(got, got.T) and np.array_equal(np.diagonal(got), counts.astype(np.uint32)) and counts.min() >= 0 and counts.any()
        sp = d.db2db_sparse(d)
        rp, col, val = D.csr_of(exp)
        assert np.array_equal(sp.row_ptr, rp) and np.array_equal(sp.col, col) and np.array_equal(sp.val, val)
        assert d.db2db_stats()["tiles_touched"] == D.tiles_of(exp)
        _same(d.db2db(d), exp, "Zself, second call")
    finally:
        d.close()
