"""new2all -sparse compacted and filtered on the device: kmdb_new2all_batch_sparse_filtered and its relatives — one2all_sp followed by the
CombinedFilter of the query's row (reference src/similarity_calculator.cpp:929-1051, src/console_new2all.cpp:76-78, 130-148).  Expected values never
come from the path under test: they are the reference's recorded rows (tests/golden), the CPU oracle's one2all, and kmdbh_metric with
a = the QUERY's k-mer count and b = the database sample's."""
import ctypes
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FMAX = float(np.finfo(np.float64).max)
ENTRIES = ["kmdb_new2all_batch_sparse_filtered", "kmdb_new2all_batch_seq_alphabet_sparse_filtered", "kmdb_new2all_rows_sparse_device",
           "kmdb_new2all_sparse_stats_get", "kmdb_node_new2all_batch_sparse_filtered", "kmdb_node_new2all_batch_seq_alphabet_sparse_filtered",
           "kmdb_node_new2all_sparse_stats_get"]
SEG = 2048                                                       # columns per segment of the compaction kernel (new2all_sparse.hip)


def mash_of(q, k):
    """the mash distance of a ratio q (reference src/params.cpp:14-42): -(1/k) ln(2 q / (1 + q))"""
    return -math.log(2.0 * q / (1.0 + q)) / k


MQ = mash_of(0.995, 18)
JAC, NUM, MASHQ = [("jaccard", 0.99, None)], [("num-kmers", 29600.0, 29750.0)], [("mash-query", None, MQ)]


def rows_of(sp):
    return [list(zip(*(a.tolist() for a in sp.row(i)))) for i in range(sp.n_rows)]


def nonzeros(dense, keep=None):
    """the rows (col, val) of dense rows, ascending columns; keep: a boolean mask of the cells to list"""
    m = dense != 0 if keep is None else (dense != 0) & keep
    return [[(int(c), int(dense[r, c])) for c in np.flatnonzero(m[r])] for r in range(dense.shape[0])]


def metric_cells(K, name, dense, a, b, k):
    """kmdbh_metric of every non-zero cell with the QUERY's count first (NaN where the cell is zero)"""
    L = K.lib()
    m = K.capi.METRICS.index(name)
    out = np.full(dense.shape, np.nan)
    for r, c in zip(*np.nonzero(dense)):
        out[r, c] = L.kmdbh_metric(m, int(dense[r, c]), int(a[r]), int(b[c]), int(k))
    return out


def expected_keep(K, dense, a, b, k, filters, swap=False):
    """the cells that pass every bound, decided by kmdbh_metric; swap: with the SAMPLE's count as a (the wrong order)"""
    keep = dense != 0
    for name, lo, hi in filters:
        x = metric_cells(K, name, dense.T, b, a, k).T if swap else metric_cells(K, name, dense, a, b, k)
        with np.errstate(invalid="ignore"):
            keep &= (x >= (-FMAX if lo is None else lo)) & (x <= (FMAX if hi is None else hi))
    return keep


class Virus:
    """virus part 2 (65 queries) against virus_k18_part1.db (100 samples): the reference's recorded rows, the queries as k-mer lists and as text"""

    def __init__(self, K, O, golden_dir):
        self.path = os.path.join(golden_dir, "virus_k18_part1.db")
        self.h = K.HostDB(self.path)
        self.k = self.h.k
        self.b = self.h.sample_kmers.astype(np.uint32)
        cwd = os.getcwd()
        os.chdir(golden_dir)
        try:
            self.qs = [km for _, km in O.load_samples(os.path.join(golden_dir, "virus.seqs.part2.list"), 18, unique=True)]
        finally:
            os.chdir(cwd)
        self.a = np.array([q.size for q in self.qs], np.uint32)
        self.dense = np.fromfile(os.path.join(golden_dir, "virus_k18_part1.n2a_part2.ref.u32"), dtype=np.uint32).reshape(65, 100)
        self.dense.setflags(write=False)
        self.sp_lines = open(os.path.join(golden_dir, "virus_k18_part1.n2a_part2_sp.ref.txt"), "rb").read().split(b"\n")
        self.texts = _virus_texts(golden_dir, "virus.seqs.part2.list")

    def keep(self, K, filters, swap=False):
        return expected_keep(K, self.dense, self.a, self.b, self.k, filters, swap)


def _virus_texts(golden_dir, list_name):
    texts = []
    with open(os.path.join(golden_dir, list_name)) as f:
        entries = [ln.strip() for ln in f if ln.strip()]
    for e in entries:
        raw = open(os.path.join(golden_dir, e + ".fasta")).read()
        recs = [r.split("\n", 1)[1] if "\n" in r else "" for r in raw.split(">") if r]
        texts.append("\n".join(r.replace("\n", "").replace("\r", "") for r in recs))
    return texts


@pytest.fixture(scope="module")
def virus(K, O, golden_dir):
    return Virus(K, O, golden_dir)


# ------------------------------------------------------------------------------------------------ CPU
def test_abi_and_argument_checks(K):
    """1. the seven entry points are exported and declared, the header announces them, the ABI version stays 8; what an entry refuses on its
    arguments it refuses under its own name, with handles that are never looked at"""
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    for name in ENTRIES:
        assert name in K.capi.EXPORTS and name + "(" in header and hasattr(L, name), name
    assert "#define KMDB_HAS_NEW2ALL_SPARSE_FILTERED 1" in header and "#define KMDB_ABI_VERSION 8" in header
    assert L.kmdb_abi_version() == 8 and K.capi.ABI_VERSION == 8
    raw = K.capi._Sparse()
    fake = ctypes.create_string_buffer(1 << 16)                  # stands for a handle: a call refused on its arguments never reads it
    h = ctypes.cast(fake, ctypes.c_void_p)
    cnt = np.ones(4, np.uint32)
    sk = cnt.ctypes.data
    u64 = np.zeros(4, np.uint64)
    one = K.capi._filters([("jaccard", 0.5, None)])
    bad = K.capi._filters([("jaccard", 0.5, None)])
    bad[0].metric = 99
    many = K.capi._filters([("jaccard", 0.0, None)] * 13)
    out = ctypes.byref(raw)
    # (filters, n_filters, sample_kmers, measure) -> what the message says
    cases = [(one, 1, None, -1, "null argument"), (None, 0, None, 5, "null argument"), (None, 0, sk, 99, "unknown measure"), (bad, 1, sk, -1, "unknown metric"),
             (many, 13, sk, -1, "more than 12 bounds")]
    calls = {
        ENTRIES[0]: lambda hd, o, f, n, s, m: L.kmdb_new2all_batch_sparse_filtered(hd, None, None, 0, f, n, s, m, o, None),
        ENTRIES[1]: lambda hd, o, f, n, s, m: L.kmdb_new2all_batch_seq_alphabet_sparse_filtered(hd, None, None, 0, 1.0, 0.0, 0, f, n, s, m, o, u64.ctypes.data, None),
        ENTRIES[2]: lambda hd, o, f, n, s, m: L.kmdb_new2all_rows_sparse_device(hd, None, 0, 0, 0, sk, f, n, s, m, o, None),
        ENTRIES[4]: lambda hd, o, f, n, s, m: L.kmdb_node_new2all_batch_sparse_filtered(hd, None, None, 0, f, n, s, m, o, None),
        ENTRIES[5]: lambda hd, o, f, n, s, m: L.kmdb_node_new2all_batch_seq_alphabet_sparse_filtered(hd, None, None, 0, 1.0, 0.0, 0, f, n, s, m, o, u64.ctypes.data, None),
    }
    for name, call in calls.items():
        for hd, o in ((None, out), (h, None)):
            assert call(hd, o, None, 0, None, -1) != 0, name
            msg = L.kmdb_last_error().decode()
            assert msg.startswith(name + ":") and "null argument" in msg, msg
        for fs, n, s, measure, what in cases:
            assert call(h, out, fs, n, s, measure) != 0, (name, what)
            msg = L.kmdb_last_error().decode()
            assert msg.startswith(name + ":") and what in msg, msg
    assert L.kmdb_new2all_rows_sparse_device(h, None, 4, 9, 3, None, None, 0, None, -1, out, None) != 0
    msg = L.kmdb_last_error().decode()
    assert msg.startswith(ENTRIES[2] + ":") and "cell_lo > cell_hi" in msg, msg
    for name, fn in ((ENTRIES[3], L.kmdb_new2all_sparse_stats_get), (ENTRIES[6], L.kmdb_node_new2all_sparse_stats_get)):
        assert fn(None, None) != 0 and L.kmdb_last_error().decode().startswith(name + ":")


def test_the_goldens_hold_what_the_gpu_tests_expect(K, virus):
    """the bounds of tests 3, 4, 7 and 8 decided on the CPU from the reference's recorded rows: each keeps some and drops some of the 6500 cells"""
    v = virus
    assert int((v.dense != 0).sum()) == 6500 and len(v.qs) == 65 and v.b.size == 100
    kj = v.keep(K, JAC)
    assert int(kj.sum()) == 2891 and int((~kj.any(axis=1)).sum()) == 1
    assert int(v.keep(K, NUM).sum()) == 4070
    kq = v.keep(K, MASHQ)
    assert int(kq.sum()) == 2377 and (kq != v.keep(K, MASHQ, swap=True)).any()


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def S(K):
    return importlib.import_module("kmerdb_amd.synth")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


@pytest.fixture(scope="module")
def vdev(K, virus, dev):
    d = K.DeviceDB(virus.h, device=dev, with_hashtables=True)
    yield d
    d.close()


@pytest.mark.gpu
def test_the_references_own_rows(K, virus, vdev):
    """2. the 65 queries as k-mer lists, no bounds: the reference's recorded one2all_sp rows line for line, the non-zeros of its dense rows; the stats"""
    v = virus
    for sp in (vdev.new2all_sparse_filtered(v.qs), vdev.new2all_sparse(v.qs)):
        assert sp.n_rows == 65 and sp.nnz == 6500 and sp.measure is None
        got = ["".join("%d:%d," % (c + 1, x) for c, x in row).encode() for row in rows_of(sp)]
        assert got == v.sp_lines[:65]
        assert rows_of(sp) == nonzeros(v.dense)
        st = vdev.new2all_sparse_stats()
        print(st)
        assert st["cells"] == 6500 and st["nnz_device"] == st["nnz"] == 6500 and st["d2h_bytes"] == 8 * 66 + 8 * 6500 and st["compact_ms"] > 0


def check_filtered(K, v, d, filters, measure=None):
    keep = v.keep(K, filters)
    n_keep, n_nz = int(keep.sum()), int((v.dense != 0).sum())
    print("%s: keeps %d of %d" % (filters, n_keep, n_nz))
    assert 0 < n_keep < n_nz, "vacuous bound %s" % (filters,)
    sp = d.new2all_sparse_filtered(v.qs, filters, v.b, measure=measure)
    assert rows_of(sp) == nonzeros(v.dense, keep), filters
    st = d.new2all_sparse_stats()
    assert st["nnz"] == n_keep == sp.nnz and st["nnz"] <= st["nnz_device"] <= n_nz and st["d2h_bytes"] == 8 * 66 + 8 * st["nnz_device"]
    return sp, keep, st


@pytest.mark.gpu
def test_bounds_query_count_first(K, virus, vdev):
    """3. every bound against kmdbh_metric(metric, c, a = the query's count, b = the sample's count, 18) on the reference's rows"""
    v = virus
    sp, keep, st = check_filtered(K, v, vdev, JAC)
    assert int(keep.sum()) == 2891 and st["nnz_device"] < 6500            # the device dropped cells
    empty = np.flatnonzero(~keep.any(axis=1))
    assert empty.size == 1 and sp.row_ptr[empty[0]] == sp.row_ptr[empty[0] + 1]
    assert int(check_filtered(K, v, vdev, NUM)[1].sum()) == 4070
    sp, keep, st = check_filtered(K, v, vdev, MASHQ)
    assert int(keep.sum()) == 2377
    swapped = v.keep(K, MASHQ, swap=True)
    assert (keep != swapped).any() and rows_of(sp) != nonzeros(v.dense, swapped)
    # two bounds together and a measure: the medians / quartiles of the two measures over the cells
    ani = metric_cells(K, "ani", v.dense, v.a, v.b, v.k)
    mx = metric_cells(K, "max", v.dense, v.a, v.b, v.k)
    sp, keep, st = check_filtered(K, v, vdev, [("ani", float(np.nanmedian(ani)), None), ("max", None, float(np.nanquantile(mx, 0.75)))], measure="ani")
    want = np.array([ani[r, c] for r in range(65) for c in np.flatnonzero(keep[r])])
    assert sp.measure is not None and sp.measure.tobytes() == want.tobytes()
    # a bound placed exactly on one cell's value keeps that cell, from either side
    jac = metric_cells(K, "jaccard", v.dense, v.a, v.b, v.k)
    mqs = metric_cells(K, "mash-query", v.dense, v.a, v.b, v.k)
    for r, c in ((64, 99), (0, 0), (31, 57)):
        for fl in ([("jaccard", float(jac[r, c]), None)], [("jaccard", None, float(jac[r, c]))], [("mash-query", None, float(mqs[r, c]))],
                   [("mash-query", float(mqs[r, c]), None)]):
            got = rows_of(vdev.new2all_sparse_filtered(v.qs, fl, v.b))
            assert (c, int(v.dense[r, c])) in got[r], (r, c, fl)
            assert got == nonzeros(v.dense, v.keep(K, fl)), (r, c, fl)


@pytest.mark.gpu
def test_text_entry(K, virus, vdev):
    """4. the same 65 queries as sequence text: the same rows, the extractor's counts, the same set under the jaccard bound"""
    v = virus
    sp, cnt = vdev.new2all_seq_sparse(v.texts)
    assert rows_of(sp) == nonzeros(v.dense) and np.array_equal(cnt, v.a.astype(np.uint64))
    st = vdev.new2all_sparse_stats()
    assert st["nnz_device"] == st["nnz"] == 6500 and st["d2h_bytes"] == 8 * 66 + 8 * 6500
    sp, cnt = vdev.new2all_seq_sparse(v.texts, JAC, v.b)
    assert rows_of(sp) == nonzeros(v.dense, v.keep(K, JAC)) and np.array_equal(cnt, v.a.astype(np.uint64))
    assert vdev.new2all_sparse_stats()["nnz_device"] < 6500


def _synth_db(S, g, ids, k, path, device):
    """database (with hashtables) of the samples `ids` of the genome model g, written in kmer-db's format"""
    pat = S.build_patterns(lambda i: S.kmers_of(g.sample(ids[i]), k), len(ids), device)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    S.write_db(path, k, 1.0, [g.name(i) for i in ids], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)


class Synth:
    """a synthetic database, queries of its model, and the ORACLE's rows — computed once, never written to"""

    def __init__(self, K, O, S, dev, tmp, N, L, r1, queries):
        import torch
        device = torch.device("cuda", dev)
        k = 18
        g = S.CladeGenomes(N, 50, L, r1=r1, r2=0.01, seed=11, device=device)
        other = S.CladeGenomes(50, 50, L, r1=r1, r2=0.01, seed=977, device=device)
        path = str(tmp / "synth.db")
        _synth_db(S, g, list(range(N)), k, path, device)
        self.qs = []
        for kind, x in queries:
            if kind == "empty":
                self.qs.append(np.zeros(0, np.uint64))
                continue
            codes = g.strain(x, N + 100 + len(self.qs)) if kind == "strain" else g.sample(x) if kind == "member" else other.sample(x)
            self.qs.append(S.kmers_of(codes, k).cpu().numpy().view(np.uint64).copy())
        h = K.HostDB(path)
        self.N, self.k = N, k
        self.a = np.array([q.size for q in self.qs], np.uint32)
        self.b = h.sample_kmers.astype(np.uint32)
        self.d = K.DeviceDB(h, device=dev, with_hashtables=True)
        o = O.OracleDB(path)
        self.dense = np.stack([o.one2all(q) for q in self.qs])
        self.dense.setflags(write=False)

    def keep(self, K, filters):
        return expected_keep(K, self.dense, self.a, self.b, self.k, filters)


N75 = 2100     # above a segment of 2048, 2100 = 32 * 64 + 52; clade 40 = ids 2000 - 2049 straddles the boundary, clade 41 = 2050 - 2099 fills the last group
Q75 = [("strain", 0), ("strain", 40), ("strain", 41), ("member", 7), ("empty", 0), ("member", 2010), ("member", 2077), ("other", 3)]


@pytest.fixture(scope="module")
def clade75(K, O, S, dev, tmp_path_factory):
    return Synth(K, O, S, dev, tmp_path_factory.mktemp("n2s75"), N75, 300, 0.75, Q75)


@pytest.mark.gpu
def test_segments_and_partial_groups(K, O, S, dev, clade75, tmp_path):
    """5. 2100 samples = a full segment and one of 52 columns: a clade across the segment boundary, a clade wholly inside the last partial group of 64,
    an empty row, an empty query between two others; then a database whose rows are mostly non-zero under bounds that cut deep"""
    c = clade75
    assert N75 > SEG and N75 % 64 and c.dense.shape == (8, N75)
    want = nonzeros(c.dense)
    cols = [set(x for x, _ in row) for row in want]
    print("non-zeros per row:", [len(x) for x in cols])
    for r in (1, 5):                                              # the straddling clade: columns on both sides of the boundary
        assert any(x < SEG for x in cols[r]) and any(x >= SEG for x in cols[r])
    for r in (2, 6):                                              # the last clade: columns of the last partial group
        assert cols[r] and all(x >= 64 * (N75 // 64) for x in cols[r])
    assert cols[0] and cols[3] and max(cols[0]) < 64 and not cols[4] and not cols[7] and c.a[4] == 0 and c.a[7] > 0
    sp = c.d.new2all_sparse_filtered(c.qs)
    assert rows_of(sp) == want
    st = c.d.new2all_sparse_stats()
    nnz = int((c.dense != 0).sum())
    assert st["cells"] == 8 * N75 and st["nnz_device"] == st["nnz"] == nnz and st["d2h_bytes"] == 8 * 9 + 8 * nnz < 4 * 8 * N75
    assert rows_of(c.d.new2all_sparse(c.qs)) == want
    # r1 = 0.10: every clade shares k-mers with every other
    w = Synth(K, O, S, dev, tmp_path, 300, 1500, 0.10, [("strain", 0), ("member", 70), ("strain", 3), ("empty", 0), ("member", 299), ("strain", 5), ("other", 1)])
    nz = int((w.dense != 0).sum())
    print("r1 = 0.10: %d non-zero cells of %d" % (nz, w.dense.size))
    assert rows_of(w.d.new2all_sparse_filtered(w.qs)) == nonzeros(w.dense)
    for fl in ([("jaccard", 0.3, None)], [("num-kmers", float(np.median(w.dense[w.dense != 0])) + 0.5, None)]):
        keep = w.keep(K, fl)
        print("%s: keeps %d of %d" % (fl, int(keep.sum()), nz))
        assert 0 < int(keep.sum()) < nz, "vacuous bound %s" % (fl,)
        assert rows_of(w.d.new2all_sparse_filtered(w.qs, fl, w.b)) == nonzeros(w.dense, keep), fl
        st = w.d.new2all_sparse_stats()
        assert st["nnz"] == int(keep.sum()) <= st["nnz_device"] < nz
    w.d.close()


@pytest.mark.gpu
def test_flat_ranges(K, dev, clade75):
    """6. the rows of test 5 accumulated by new2all_device into a zeroed buffer, compacted range by range: cuts inside a group of 64 of a row, on a
    row boundary and inside the last partial group of a row, one range empty; the parts concatenate row by row to the whole, with a bound as well"""
    import torch
    c = clade75
    N, nq = N75, len(c.qs)
    buf = torch.zeros((nq, N), dtype=torch.int32, device=torch.device("cuda", dev))
    c.d.new2all_device(c.qs, buf.data_ptr())
    torch.cuda.synchronize()
    cuts = [0, 1 * N + 2030, 3 * N, 6 * N + 2070, 6 * N + 2070, nq * N]
    assert c.dense[1, 2030 - 30:2030].any() and c.dense[1, 2030:2048].any() and c.dense[6, 2050:2070].any() and c.dense[6, 2070:].any()
    jac = metric_cells(K, "jaccard", c.dense, c.a, c.b, c.k)
    bound = [("jaccard", float(np.nanmedian(jac)), None)]
    keep = c.keep(K, bound)
    assert 0 < int(keep.sum()) < int((c.dense != 0).sum())
    whole = c.d.new2all_rows_sparse_device(buf.data_ptr(), nq)
    assert rows_of(whole) == nonzeros(c.dense)
    for fl, want in (((), nonzeros(c.dense)), (bound, nonzeros(c.dense, keep))):
        got = [[] for _ in range(nq)]
        cells = 0
        for lo, hi in zip(cuts, cuts[1:]):
            sp = c.d.new2all_rows_sparse_device(buf.data_ptr() + 4 * lo, nq, lo, hi, c.a, fl, c.b if fl else None)
            st = c.d.new2all_sparse_stats()
            assert sp.n_rows == nq and st["cells"] == hi - lo and st["d2h_bytes"] == 8 * (nq + 1) + 8 * st["nnz_device"]
            part = rows_of(sp)
            for r in range(nq):
                assert all(lo <= r * N + col < hi for col, _ in part[r]), (lo, hi, r)
                got[r] += part[r]
            if lo == hi:
                assert sp.nnz == 0 and not sp.row_ptr.any()
            cells += st["cells"]
        assert got == want and cells == nq * N, fl
    with pytest.raises(K.KmdbError, match="kmdb_new2all_rows_sparse_device: cell_hi beyond"):
        c.d.new2all_rows_sparse_device(buf.data_ptr(), nq, 0, nq * N + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("force_rccl", [False, True])
def test_node(K, virus, dev, golden_dir, force_rccl, monkeypatch):
    """7. three query shards on one device (and the same with the reduce-scatter on a one-rank communicator): the rows of tests 2 - 4, k-mer and text
    entry, with and without the jaccard bound; refusals under the new entry points' names"""
    if force_rccl:
        monkeypatch.setenv("KMDB_NODE_FORCE_RCCL", "1")
    v = virus
    keep = v.keep(K, JAC)
    nd = K.NodeDB(v.h, 3, [dev], partition="prefix-tables")
    assert rows_of(nd.new2all_sparse(v.qs)) == nonzeros(v.dense)
    st = nd.new2all_sparse_stats()
    assert st["cells"] == 6500 and st["nnz_device"] == st["nnz"] == 6500 and st["d2h_bytes"] == 8 * 66 + 8 * 6500 and st["compact_ms"] > 0
    assert rows_of(nd.new2all_sparse(v.qs, JAC, v.b)) == nonzeros(v.dense, keep)
    st = nd.new2all_sparse_stats()
    assert st["nnz"] == 2891 <= st["nnz_device"] < 6500
    sp, cnt = nd.new2all_seq_sparse(v.texts)
    assert rows_of(sp) == nonzeros(v.dense) and np.array_equal(cnt, v.a.astype(np.uint64))
    sp, cnt = nd.new2all_seq_sparse(v.texts, JAC, v.b, measure="jaccard")
    assert rows_of(sp) == nonzeros(v.dense, keep) and np.array_equal(cnt, v.a.astype(np.uint64))
    jac = metric_cells(K, "jaccard", v.dense, v.a, v.b, v.k)
    assert sp.measure.tobytes() == np.array([jac[r, c] for r in range(65) for c in np.flatnonzero(keep[r])]).tobytes()
    assert nd.stats()["call_ms"] > 0 and (nd.stats()["collective_ms"] > 0) == force_rccl
    nd.close()
    if force_rccl:
        return
    pre = K.NodeDB(v.h, 2, [dev], partition="prefix")
    with pytest.raises(K.KmdbError, match="kmdb_node_new2all_batch_sparse_filtered: the node was uploaded with partition prefix;"):
        pre.new2all_sparse(v.qs[:2], JAC, v.b)
    with pytest.raises(K.KmdbError, match="kmdb_node_new2all_batch_seq_alphabet_sparse_filtered: the node was uploaded with partition prefix;"):
        pre.new2all_seq_sparse(v.texts[:2])
    pre.close()
    shard = K.DeviceDB(v.h, device=dev, query_shard=(0, 2))
    with pytest.raises(K.KmdbError, match="kmdb_new2all_batch_sparse_filtered: a query shard"):
        shard.new2all_sparse_filtered(v.qs[:2], JAC, v.b)
    with pytest.raises(K.KmdbError, match="kmdb_new2all_batch_seq_alphabet_sparse_filtered: a query shard"):
        shard.new2all_seq_sparse(v.texts[:2])
    shard.close()
    bare = K.DeviceDB(K.HostDB(v.path, skip_hashtables=True), device=dev)
    with pytest.raises(K.KmdbError, match="kmdb_new2all_batch_sparse_filtered: database was uploaded without hashtables"):
        bare.new2all_sparse_filtered(v.qs[:2])
    bare.close()


def _cli(*args, env=None):
    exe = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=None if env is None else dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.gpu
def test_front_end(K, golden_dir, dev, tmp_path):
    """8. `new2all -sparse` with a bound == the lines of the reference's unfiltered table (golden virus.k18.n2a.sparse.csv) with every col:val kept or
    dropped by kmdbh_metric and the counts on the file's own lines; the same bytes with the dense rows, the host's extractor and -gpus 2"""
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    L = K.lib()
    golden = open(g("virus.k18.n2a.sparse.csv"), "rb").read()
    lines = golden.split(b"\n")
    counts = [int(x) for x in lines[1].split(b",")[2:] if x]
    assert lines[1].startswith(b"query-samples,total-kmers,") and len(counts) == 100
    LINE = "[kmdb] new2all: sparse batch of"
    cwd = os.getcwd()
    os.chdir(golden_dir)          # list entries are ./test/virus/data/<name>
    try:
        for tag, opt, metric, lo, hi in (("minj", ["-min", "jaccard:0.99"], "jaccard", 0.99, FMAX), ("maxq", ["-max", "mash-query:%r" % MQ], "mash-query", -FMAX, MQ)):
            m = K.capi.METRICS.index(metric)
            want, kept, seen = lines[:2], 0, 0
            for ln in lines[2:]:
                if not ln:
                    want.append(ln)
                    continue
                f = ln.split(b",")
                cells = []
                for cv in f[2:-1]:
                    c, v = (int(x) for x in cv.split(b":"))
                    seen += 1
                    if lo <= L.kmdbh_metric(m, v, int(f[1]), counts[c - 1], 18) <= hi:
                        cells.append(cv)
                kept += len(cells)
                want.append(b",".join(f[:2] + cells + [b""]))
            print("%s: keeps %d of %d pairs" % (tag, kept, seen))
            assert 0 < kept < seen
            want = b"\n".join(want)
            for name, extra, env in (("dev", [], None), ("dense", [], {"KMDB_N2A_DENSE_ROWS": "1"}), ("host", ["-host-extract"], None), ("g2", ["-gpus", "2"], None)):
                out = t("%s.%s.csv" % (tag, name))
                _cli("new2all", "-sparse", *opt, *extra, g("virus_k18_part1.db"), g("virus.seqs.part2.list"), out, env=env)
                assert open(out, "rb").read() == want, (tag, name)
        for name, extra, env, line in (("plain", [], {"KMDB_VERBOSE": "1"}, True), ("plain.dense", [], {"KMDB_VERBOSE": "1", "KMDB_N2A_DENSE_ROWS": "1"}, False),
                                       ("plain.g2", ["-gpus", "2"], {"KMDB_VERBOSE": "1"}, True)):
            r = _cli("new2all", "-sparse", *extra, g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t(name), env=env)
            assert open(t(name), "rb").read() == golden, name
            assert (LINE in r.stderr) == line, (name, r.stderr)
    finally:
        os.chdir(cwd)
