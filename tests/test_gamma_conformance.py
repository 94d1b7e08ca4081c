"""Gamma-stream decode conformance: every stream reader of the engine — RunCursor32 (all2all's decode kernel, short and long launch),
GammaCursor<2> (the v1 kernels, the upload's estimates, new2all's checkpoints) and GammaCursor<1> (new2all's run index, walk and queued
lists; db2db's list store and root-path climb) — meets every code length at every bit offset, lists either side of the 128-bit bound
of the short launch, of every 32nd id (new2all's checkpoints), of the longest run the run index stores, and of 65 536 ids (31 / 33-bit
codes).  The inputs are tests/gamma_cases.py's; a census on the host proves what they hold before a device runs.  The references are the
decoded lists themselves (variant_cases.definition, its sparse form, one2all_from_lists, db2db_from_lists) and the CPU oracle, never a
second run of the engine; all comparisons are exact uint32 equality.

What cannot be reached: codes of 35 to 39 bits in RunCursor32 (all2all would need more than 131 072 samples: a 34 GB matrix); they are
decoded by GammaCursor<1> and GammaCursor<2> in collection D (526 336 samples).  A change to any reader must pass this file."""
import functools
import os

import numpy as np
import pytest

import gamma_cases as G
import variant_cases as V
from test_gpu_parity import _Laps
from test_kernel_variants import SWITCHES, _oracle_of, _S, _same


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


@pytest.fixture
def env(monkeypatch):
    """set(name=value, ...) replaces ALL of the engine's switches by the ones given"""
    def set_(**kw):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in kw.items():
            assert name in SWITCHES, name
            monkeypatch.setenv(name, str(value))
    set_()
    return set_


class _Lap(_Laps):
    """the laps of _Laps, printed as well (pytest -s / the captured output of a failing test)"""

    def done(self):
        print(self.name + " " + " ".join(self.laps), flush=True)
        super().done()


@functools.lru_cache(maxsize=None)
def _arrays(name):
    pat, tags, N = G.collection(name)
    return _S().to_view_arrays(pat)


@functools.lru_cache(maxsize=None)
def _case_A():
    """collection A, its definition (== the oracle, test_references_agree) — computed once, never written to"""
    pat, tags, N = G.collection("A")
    exp = V.definition(pat, N)
    exp.setflags(write=False)
    return pat, N, exp


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "R16"])
def test_independent_coder_equals_the_synth_encoder(K, name):
    """synth.to_view_arrays (gamma_encode_patterns: the encoder every other test relies on) against the big-integer coder of
    gamma_cases.py, per list: the same words, num_bits and last_sample_id; the whole data array byte for byte; and the coder's own
    round trip back to the ids"""
    pat, tags, N = G.collection(name)
    arr = _arrays(name)
    lp, ids = pat["local_ptr"].numpy(), pat["local_ids"].numpy()
    data = []
    for p, (words, nb, l, last) in enumerate(G.streams(arr)):
        loc = ids[lp[p]: lp[p + 1]]
        assert l == loc.size
        mine, bits = G.encode(np.diff(loc).tolist())
        assert bits == nb and mine == words, (name, p, tags[p])
        assert int(arr["data_offset"][p]) == len(data)
        data += mine
        if l:
            assert last == loc[-1] and G.decode(mine, bits, l, last) == loc.tolist(), (name, p, tags[p])
    assert np.array(data + [0, 0], dtype=np.uint64).tobytes() == arr["data"].tobytes()
    assert arr["num_bits"].dtype == np.uint32 and arr["last_sample_id"].dtype == np.uint32 and arr["data"].dtype == np.uint64


ALL64 = set(range(64))


def test_census_of_the_collections():
    """What the decoded streams hold, before any device runs.  A: every code length 3 .. 23 at every offset mod 64 from its stream's start,
    once at the head of a step (no "0" code before it) and once behind zeros — by the align lists' own code; a run of zeros longer than
    two windows; streams of 127 / 128 / 129 bits among the lists of at most 48 ids and lists of 49 ids; every checkpoint length; ids 0
    and N - 1.  B, D: every length of the collection at every offset over the two kinds.  C: 65 535 and 65 536 side by side, every offset
    of a 32-bit unit behind zeros, 20 offsets and more at the head.  D and R16: the runs either side of the run index's longest."""
    c = {name: G.census(_arrays(name), G.SIZES[name], G.collection(name)[1]) for name in G.SIZES}
    for name, N in G.SIZES.items():
        assert c[name]["ids"] == (0, N - 1), name
        assert {127, 128, 129} <= c[name]["bits_short"] and 49 in c[name]["lengths"], name
        assert N - 1 in c[name]["deltas"], name
    a = c["A"]["aligned"]
    for j in G.JS["A"]:
        assert a[2 * j + 1]["head"] == ALL64 and a[2 * j + 1]["behind"] == ALL64, (j, ALL64 - a[2 * j + 1]["head"], ALL64 - a[2 * j + 1]["behind"])
    assert all(d in c["A"]["deltas"] for j in range(1, 11) for d in G.D_of(j)) and 1 << 11 in c["A"]["deltas"]
    assert c["A"]["longest_zero_run"] >= 64 + 40
    assert set(G.CHECKPOINT_LENGTHS) | {200, 333, 450, 600} <= c["A"]["lengths"]
    tags = G.collection("A")[1]
    assert ("run end", 4095, "root") in tags and ("run end", 4094, "root") in tags
    for name in ("B", "D"):
        a = c[name]["aligned"]
        for j in G.JS[name]:
            assert a[2 * j + 1]["head"] | a[2 * j + 1]["behind"] == ALL64, (name, j)
            assert len(a[2 * j + 1]["head"]) >= 32 and len(a[2 * j + 1]["behind"]) >= 32, (name, j)
        assert set(G.CHECKPOINT_LENGTHS) <= c[name]["lengths"], name
    assert {1 << 15, 65534} <= c["B"]["deltas"] and max(c["B"]["deltas"]) == 65534
    assert {65535, 65536, 65537, 65590} <= c["C"]["deltas"]
    for ln in (31, 33):
        a = c["C"]["aligned"][ln]
        assert {x % 32 for x in a["behind"]} == set(range(32)) and len(a["head"]) >= 20, (ln, a)
    assert {1 << 16, 1 << 17, 1 << 18, 1 << 19} <= c["D"]["deltas"] and {31, 33, 35, 37, 39} <= set(c["D"]["offsets"])
    # the runs: one run of max_len - 1 .. 2 max_len + 1 ids (4095 above 65 536 samples, 65 535 up to there)
    assert {4094, 4095, 4096, 8191} <= c["D"]["lengths"] and c["D"]["longest_zero_run"] == 8190
    assert {65534, 65535, 65536} <= c["R16"]["lengths"] and c["R16"]["longest_zero_run"] == 65535


def _queries(kmers, pids, absent):
    """queries over a fabricated dictionary: the k-mers of every third pattern (three of them: every list gets a count from one, its
    neighbours other counts), all k-mers, absent k-mers only, one k-mer, none"""
    qs = [kmers[pids % 3 == r] for r in range(3)]
    return qs + [kmers.copy(), np.sort(absent[:200]), kmers[:1].copy(), np.zeros(0, np.uint64)]


class _Db:
    """a case collection as a database with a fabricated dictionary: forest, .db file, host and oracle handles, queries"""

    def __init__(self, K, O, name, N, folder, column_of=None):
        import torch
        S = _S()
        k = 18
        if column_of is None:
            pat, _, _ = G.collection(name)
            self.pat, self.kmers, self.pids, self.absent = G.with_dictionary(pat, 1000 + len(name))
        else:
            # the column part: every k-mer of the row part and 300 of its own, spread over the column forest's patterns
            pat = G.column_forest()
            P = int(pat["parent"].numel())
            kmers = np.concatenate([column_of.kmers, column_of.absent[200:500]])
            order = np.argsort(kmers)
            self.kmers = kmers[order]
            self.pids = (1 + np.arange(kmers.size) % (P - 1))[order]
            self.pat = dict(pat)
            self.pat["num_kmers"] = torch.from_numpy(np.bincount(self.pids, minlength=P).astype(np.int64))
            self.absent = column_of.absent[:200]
        self.N = N
        arr = S.to_view_arrays(self.pat)
        tables = S.build_hashtables(torch.from_numpy(self.kmers.astype(np.int64)), torch.from_numpy(self.pids.astype(np.int64)), k)
        self.path = os.path.join(folder, "%s_%d%s.db" % (name, N, "_col" if column_of else ""))
        S.write_db(self.path, k, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr, kmers_count=int(self.kmers.size), tables=tables)
        self.host = K.HostDB(self.path)
        self.oracle = O.OracleDB(self.path)
        self.queries = _queries(self.kmers, self.pids, self.absent)

    @functools.lru_cache(maxsize=None)
    def rows(self):
        exp = np.stack([self.oracle.one2all(q) for q in self.queries])
        exp.setflags(write=False)
        return exp


@pytest.fixture(scope="module")
def dbs(K, O, tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("gamma"))
    made = {}

    def get(name, N=None, column_of=None):
        key = (name, N or G.SIZES[name], column_of is not None)
        if key not in made:
            made[key] = _Db(K, O, name, key[1], folder, column_of)
        return made[key]
    return get


def test_references_agree(K, O, dbs):
    """A: the oracle's tree form == its flat form == variant_cases.definition == the sparse definition's cells.  A and D as databases:
    the oracle's one2all and db2db (a 64-sample column part, both ways round) equal the rows and the cell added up from the lists."""
    pat, N, exp = _case_A()
    tree, flat = _oracle_of(O, pat, N)
    assert np.array_equal(tree, flat) and np.array_equal(tree, exp), V.describe_mismatch(tree, exp, N)
    idx, val = G.sparse_definition(pat, N)
    nz = np.nonzero(exp)[0]
    assert np.array_equal(idx, nz) and np.array_equal(val, exp[nz])
    for name in ("A", "D"):
        db = dbs(name)
        col = dbs(name, 64, column_of=db)
        rows = db.rows()
        for qi, q in enumerate(db.queries):
            hit = db.pids[np.isin(db.kmers, q)]
            assert np.array_equal(rows[qi], G.one2all_from_lists(db.pat, db.N, hit)), (name, qi)
        assert rows[:4].any(axis=1).all() and not rows[4].any() and rows[5].any() and not rows[6].any()
        # every list gets a count from the query of all k-mers, and none of the three partial queries counts in all lists
        last = np.array([full[-1] if full.size else 0 for full in V.full_lists(db.pat)])
        assert (rows[3][last[1:]] > 0).all() and max(rows[r][last[1:]].min() for r in range(3)) == 0
        shared = np.isin(col.kmers, db.kmers)
        assert np.array_equal(col.kmers[shared], db.kmers)
        cell = G.db2db_from_lists(db.pat, db.N, db.pids, col.pat, 64, col.pids[shared])
        assert np.array_equal(db.oracle.db2db(col.oracle), cell), name
        assert np.array_equal(col.oracle.db2db(db.oracle), cell.T), name


# ------------------------------------------------------------------------------------------------------------------------------------
# all2all
# ------------------------------------------------------------------------------------------------------------------------------------
A2A_VARIANTS = [{}] + [{"KMDB_SHORT_IDS": s} for s in (1, 47, 48, 64)] + [{"KMDB_K1N_MODE": m, "KMDB_ROW_MODE": r} for m in (0, 1, 2) for r in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", A2A_VARIANTS, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) or "default")
def test_all2all_collection_a(K, dev, env, variant):
    """RunCursor32 at every code length of up to 23 bits and every offset: the whole matrix of collection A == the definition, on the
    block-record pipeline (FLAG_NO_FALLBACK; stats().path says so) with the short launch taking lists of up to 1, 47, 48 and 64 ids and
    under every first-block and row mode; in the default configuration also GammaCursor<2> in the three v1 kernels"""
    pat, N, exp = _case_A()
    lap = _Lap("all2all_collection_a %s" % variant)
    _, view = V.make_view(K, _S(), pat, N)
    env(**variant)
    d = K.DeviceDB(view, device=dev)
    got = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
    assert d.stats()["path"] == K.capi.PATH_RECORDS, d.stats()
    _same(got, exp, N, "collection A %s" % variant)
    lap("block records")
    if not variant:
        for fl, path in ((K.capi.FLAG_FORCE_TILE, K.capi.PATH_TILE), (K.capi.FLAG_FORCE_GLOBAL_ATOMICS, K.capi.PATH_GLOBAL), (K.capi.FLAG_FORCE_DIRECT, None)):
            _same(d.all2all_dense(flags=fl), exp, N, "collection A, v1 flag %d" % fl)
            assert path is None or d.stats()["path"] == path, (fl, d.stats())
        lap("v1 kernels")
    d.close()
    lap.done()


CHUNK = 1 << 30


def _check_device_matrix(M, idx_d, val_d, what):
    """M: the lower triangle on the device (int32 holding the uint32 cells).  Every expected cell holds its value; M has as many non-zero
    cells as expected; the 64-bit sum of M is the 64-bit sum of the values.  In chunks below 2^31 elements."""
    import torch
    count = total = 0
    for a in range(0, M.numel(), CHUNK):
        part = M[a: a + CHUNK]
        lo, hi = torch.searchsorted(idx_d, torch.tensor([a, a + part.numel()], device=idx_d.device)).tolist()
        got = part[idx_d[lo:hi] - a]
        bad = torch.nonzero(got != val_d[lo:hi])
        assert bad.numel() == 0, "%s: %d expected cells differ; first: cell %d got %d, expected %d" % (
            what, bad.numel(), int(idx_d[lo + int(bad[0])]), int(got[int(bad[0])]) & 0xFFFFFFFF, int(val_d[lo + int(bad[0])]) & 0xFFFFFFFF)
        count += int(torch.count_nonzero(part))
        total += int(part.sum(dtype=torch.int64)) + (int(torch.count_nonzero(part < 0)) << 32)
    assert count == idx_d.numel(), "%s: %d non-zero cells, %d expected" % (what, count, idx_d.numel())
    expected = int(val_d.sum(dtype=torch.int64)) + (int(torch.count_nonzero(val_d < 0)) << 32)
    assert total == expected, "%s: sum of the matrix %d, of the expected cells %d" % (what, total, expected)


def _big_all2all(K, dev, name, calls):
    """all2all on a collection whose matrix (8.6 GB) stays on the device, against the sparse definition.  calls(d, M, M2, check)"""
    import torch
    lap = _Lap("all2all_collection_%s" % name.lower())
    device = torch.device("cuda", dev)
    pat, tags, N = G.collection(name)
    idx, val = G.sparse_definition(pat, N)
    assert 0 < idx.size < 8_000_000 and idx[-1] < N * (N - 1) // 2
    lap("sparse definition (%d cells)" % idx.size)
    idx_d, val_d = torch.from_numpy(idx).to(device), torch.from_numpy(val.view(np.int32)).to(device)
    _, view = V.make_view(K, _S(), pat, N)
    d = K.DeviceDB(view, device=dev)
    M = torch.zeros(d.tri_size(), dtype=torch.int32, device=device)
    lap("upload, matrix")

    def check(T, what):
        torch.cuda.synchronize(device)
        lap(what)
        _check_device_matrix(T, idx_d, val_d, "collection %s, %s" % (name, what))
        lap("checked")
    try:
        calls(d, M, check)
    finally:
        d.close()
        del M
        torch.cuda.empty_cache()
        lap.done()


@pytest.mark.gpu
def test_more_than_65535_samples_gamma_collection_b(K, dev, env):
    """Codes of 25 to 31 bits — the longest of RunCursor32's 32-bit path and of the v1 kernels' 16-bit ids — at every offset, 65 535
    samples: the block-record pipeline and the three v1 kernels.  Every expected cell, the number of non-zero cells, the sum."""
    def calls(d, M, check):
        d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_NO_FALLBACK)
        assert d.stats()["path"] == K.capi.PATH_RECORDS, d.stats()
        check(M, "block records")
        for fl, what in ((K.capi.FLAG_FORCE_TILE, "v1 tile"), (K.capi.FLAG_FORCE_GLOBAL_ATOMICS, "v1 global atomics"), (K.capi.FLAG_FORCE_DIRECT, "v1 direct")):
            d.all2all_dense_device(M.data_ptr(), flags=fl)
            check(M, what)
    _big_all2all(K, dev, "B", calls)


@pytest.mark.gpu
def test_more_than_65535_samples_gamma_collection_c(K, dev, env):
    """Deltas 65 535 (31 bits: the last code of the 32-bit window) and 65 536, 65 537, 65 590 (33 bits: the 64-bit side path of
    RunCursor32::step) side by side, 65 600 samples: the block-record pipeline, two slices of the pattern stream summed, and the
    HBM-atomics kernel (GammaCursor<2>, 32-bit ids)."""
    import torch

    def calls(d, M, check):
        d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_NO_FALLBACK)
        assert d.stats()["path"] == K.capi.PATH_RECORDS, d.stats()
        check(M, "block records")
        M2 = torch.zeros_like(M)
        d.all2all_dense_device(M.data_ptr(), shard=(0, 2), flags=K.capi.FLAG_NO_FALLBACK)
        d.all2all_dense_device(M2.data_ptr(), shard=(1, 2), flags=K.capi.FLAG_NO_FALLBACK)
        for a in range(0, M.numel(), CHUNK):
            M2[a: a + CHUNK] += M[a: a + CHUNK]
        check(M2, "two slices summed")
        del M2
        d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_FORCE_GLOBAL_ATOMICS)
        assert d.stats()["path"] == K.capi.PATH_GLOBAL, d.stats()
        check(M, "v1 global atomics")
    _big_all2all(K, dev, "C", calls)


# ------------------------------------------------------------------------------------------------------------------------------------
# new2all
# ------------------------------------------------------------------------------------------------------------------------------------
N2A_VARIANTS = ({}, {"KMDB_N2A_NO_RUNS": 1}, {"KMDB_N2A_NO_NODES": 1}, {"KMDB_N2A_THREADS": 1024})


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", [("A", 4096), ("A", 10000), ("C", 65600), ("R16", 65536), ("D", G.SIZES["D"])])
def test_new2all_on_the_collections(K, O, dev, env, dbs, name, N):
    """GammaCursor<1> (next and zeros) and GammaCursor<2> in ck_fill_kernel: with the run index (n2a_runs_kernel; 16-bit starts and runs of up to
    65 535 ids at 65 536 samples, 20-bit starts and runs of up to 4095 above), without it (the inline decode of the walk, the queued long
    lists from a checkpoint: a long code directly before, on and behind every 32nd id), over the engine's arrays, and with 1024 threads.
    The per-query histogram is in LDS for A at 4096 samples, for A at 10 000 with 512 threads only, in memory for C, R16 and D.  The
    difference form of the queued lists is the LDS histogram's: A's queued lists whose last run ends at id N - 1 (no -H behind it) and
    at id N - 2 (a -H on the last id) go through it at 4096 samples; R16's and D's runs up to id N - 1 take the memory form.  Rows ==
    the oracle's one2all (== the lists: test_references_agree); the rows of new2all_sparse == their non-zeros."""
    lap = _Lap("new2all %s %d" % (name, N))
    db = dbs(name, N)
    exp = db.rows()
    assert exp[:4].any(axis=1).all()
    nz = [np.nonzero(r)[0] for r in exp]
    lap("database, oracle")
    for variant in N2A_VARIANTS:
        env(**variant)
        d = K.DeviceDB(db.host, device=dev, with_hashtables=True)
        got = d.new2all(db.queries)
        assert np.array_equal(got, exp), (name, N, variant, [int((g != e).sum()) for g, e in zip(got, exp)],
                                          [int(np.nonzero(g != e)[0][0]) if (g != e).any() else -1 for g, e in zip(got, exp)])
        sp = d.new2all_sparse(db.queries)
        assert sp.n_rows == len(db.queries)
        for qi in range(len(db.queries)):
            c, v = sp.row(qi)
            assert np.array_equal(c, nz[qi]) and np.array_equal(v, exp[qi][nz[qi]]), (name, N, variant, qi)
        assert np.array_equal(d.new2all(db.queries), exp), (name, N, variant, "second call")
        d.close()
        lap(" ".join("%s=%s" % kv for kv in variant.items()) or "default")
    lap.done()


# ------------------------------------------------------------------------------------------------------------------------------------
# db2db
# ------------------------------------------------------------------------------------------------------------------------------------
def _csr(dense):
    r, c = np.nonzero(dense)
    row_ptr = np.zeros(dense.shape[0] + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(r, minlength=dense.shape[0]))
    return row_ptr, c, dense[r, c]


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", [("A", 4096), ("A", 4097), ("D", G.SIZES["D"])])
def test_db2db_on_the_collections(K, O, dev, env, dbs, name, N):
    """GammaCursor<1>, next only (db2db): the list store (a part of 4096 samples) and the root-path climb (4097 samples, and D: codes of up to 39 bits), the case
    collection as the row part and as the column part of a cell with a 64-sample part that shares every k-mer with it.  The dense cell ==
    the oracle's db2db (== the lists: test_references_agree), the rows of db2db_sparse == its non-zeros."""
    lap = _Lap("db2db %s %d" % (name, N))
    row = dbs(name, N)
    col = dbs(name, 64, column_of=dbs(name))                      # (the dictionary is the forest's: the same at every N)
    assert np.array_equal(row.kmers, dbs(name).kmers) and np.array_equal(row.pids, dbs(name).pids)
    exp = row.oracle.db2db(col.oracle)
    assert exp.shape == (N, 64) and exp.any()
    lap("databases, oracle")
    drow = K.DeviceDB(row.host, device=dev, with_hashtables=True)
    dcol = K.DeviceDB(col.host, device=dev, with_hashtables=True)
    try:
        for a, b, e, what in ((drow, dcol, exp, "case part as rows"), (dcol, drow, np.ascontiguousarray(exp.T), "case part as columns")):
            got = a.db2db(b)
            assert got.shape == e.shape and np.array_equal(got, e), (name, N, what, int((got != e).sum()), np.argwhere(got != e)[:3].tolist())
            sp = a.db2db_sparse(b)
            rp, c, v = _csr(e)
            assert np.array_equal(sp.row_ptr, rp) and np.array_equal(sp.col, c) and np.array_equal(sp.val, v), (name, N, what, "sparse rows")
            lap(what)
    finally:
        drow.close()
        dcol.close()
    lap.done()
