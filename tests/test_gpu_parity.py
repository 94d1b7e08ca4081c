"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle and
the committed outputs of the real reference, bit-exact (all arithmetic is uint32 / integer)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DBS, ROOT

pytestmark = pytest.mark.gpu


class _Laps:
    """Where a long test spends its seconds: KMDB_TEST_PHASES=<file> appends one line per test (name, phase:seconds ...)."""

    def __init__(self, name):
        import time
        self.name, self.t, self.laps, self.clock = name, time.time(), [], time.time

    def __call__(self, phase):
        now = self.clock()
        self.laps.append("%s:%.1f" % (phase, now - self.t))
        self.t = now

    def done(self):
        path = os.environ.get("KMDB_TEST_PHASES")
        if path:
            with open(path, "a") as f:
                f.write(self.name + " " + " ".join(self.laps) + "\n")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


def _ref_dense(golden_dir, stem):
    stem = "virus_k18" if stem == "virus_k18_parts" else stem
    return np.fromfile(os.path.join(golden_dir, stem + ".a2a.ref.u32"), dtype=np.uint32)


@pytest.mark.parametrize("stem", DBS)
def test_all2all_dense_bit_exact(K, O, golden_dir, dev, stem):
    path = os.path.join(golden_dir, stem + ".db")
    h = K.HostDB(path, skip_hashtables=True)
    d = K.DeviceDB(h, device=dev)
    ref = _ref_dense(golden_dir, stem)
    got = d.all2all_dense()
    assert np.array_equal(got, ref)
    assert np.array_equal(got, O.OracleDB(path, skip_hashtables=True).all2all_dense())
    st = d.stats()
    assert st["sum_pairs"] == int(ref.astype(np.uint64).sum())
    assert st["algorithmic_bytes"] == h.pattern_section_bytes + 4 * d.tri_size()
    # idempotent: the resident db is not mutated (the reference accumulates num_kmers in place, :64-72)
    assert np.array_equal(d.all2all_dense(), ref)
    # the default path is the block-record pipeline; the second call reuses the grid sizes the first one measured
    st = d.stats()
    assert st["path"] == K.capi.PATH_RECORDS and st["sized_call"] == 0 and (st["n_records"] + st["n_direct"] > 0 or d.P <= 1)
    # a database laid out again (nothing cached) and forced to fail instead of falling back
    d2 = K.DeviceDB(h, device=dev)
    assert np.array_equal(d2.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), ref)
    assert d2.stats()["sized_call"] == 1
    d2.close()
    # a handle uploaded for a process that ends after its call (the front-end): the staging buffers stay mapped, calls are what they were
    d3 = K.DeviceDB(h, device=dev, flags=K.capi.FLAG_ONE_SHOT)
    assert np.array_equal(d3.all2all_dense(flags=K.capi.FLAG_ONE_SHOT), ref) and np.array_equal(d3.all2all_dense(), ref)
    d3.close()
    # the A/B kernels: generic (global stack + HBM atomics), LDS stack + HBM atomics, wave-private LDS tile
    for fl in (K.capi.FLAG_FORCE_GLOBAL_ATOMICS, K.capi.FLAG_FORCE_DIRECT, K.capi.FLAG_FORCE_TILE):
        assert np.array_equal(d.all2all_dense(flags=fl), ref), fl
    assert d.stats()["n_records"] == 0 and d.stats()["path"] in (K.capi.PATH_TILE, K.capi.PATH_GLOBAL)
    # unknown flag bits are rejected (they used to select timing experiments)
    with pytest.raises(K.KmdbError, match="unknown bits"):
        d.all2all_dense(flags=1 << 9)


@pytest.mark.parametrize("stem", ["virus_k18", "clade64", "clade64_k25_f01"])
@pytest.mark.parametrize("shards", [2, 3, 8])
def test_shards_sum_to_full_matrix(K, golden_dir, dev, stem, shards):
    h = K.HostDB(os.path.join(golden_dir, stem + ".db"), skip_hashtables=True)
    d = K.DeviceDB(h, device=dev)
    acc = np.zeros(d.tri_size(), dtype=np.uint32)
    for s in range(shards):
        acc += d.all2all_dense(shard=(s, shards))
        assert d.stats()["path"] == K.capi.PATH_RECORDS          # slices of the pattern stream stay on the fast path
    assert np.array_equal(acc, _ref_dense(golden_dir, stem))


def _np_metric(name, c, a, b, k):
    """the measures of params.cpp:14-42 restated with numpy (uint32 wrap-around integer parts, float64)"""
    c, a, b = c.astype(np.uint32), a.astype(np.uint32), b.astype(np.uint32)
    with np.errstate(all="ignore"):
        def mash(j):
            # math.log = the C library's log, as in the reference (numpy's vectorised log may differ in the last bit)
            r = (2 * j) / (j + 1)
            lg = np.array([math.log(x) if x > 0 and np.isfinite(x) else (float("-inf") if x == 0 else float("nan")) for x in r.tolist()])
            return np.where(j == 0, 1.0, (-1.0 / k) * lg)
        jac = c.astype(np.float64) / (a + b - c).astype(np.float64)
        mn = c.astype(np.float64) / np.minimum(a, b).astype(np.float64)
        return {"jaccard": jac, "min": mn, "max": c.astype(np.float64) / np.maximum(a, b).astype(np.float64),
                "cosine": c.astype(np.float64) / np.sqrt((a * b).astype(np.float64)), "mash": mash(jac), "ani": 1.0 - mash(jac),
                "ani-shorter": 1.0 - mash(mn), "mash-query": mash(c.astype(np.float64) / a.astype(np.float64)),
                "num-kmers": c.astype(np.float64)}[name]


@pytest.mark.parametrize("stem", ["virus_k18", "synth_k21", "clade64", "clade64_k25_f01"])
def test_all2all_sparse_filtered_on_device(K, golden_dir, dev, stem):
    """-min / -max bounds applied before the result leaves HBM, measures for the kept cells.  Against the
    unfiltered result filtered here with the restated measures: bounds taken FROM the data (so that cells sit exactly on
    them), every criterion, pairs of criteria, one-sided bounds, bounds nothing / everything passes."""
    h = K.HostDB(os.path.join(golden_dir, stem + ".db"), skip_hashtables=True)
    d = K.DeviceDB(h, device=dev)
    k = h.k
    cnt = h.sample_kmers.astype(np.uint32)
    full = d.all2all_sparse()
    rows = np.repeat(np.arange(d.N), np.diff(full.row_ptr).astype(np.int64))
    rng = np.random.default_rng(7)
    names = K.capi.METRICS
    # kmdbh_metric == the numpy restatement on every cell (libm log on both sides)
    L = K.capi.lib()
    for name in names:
        want = _np_metric(name, full.val, cnt[rows], cnt[full.col], k)
        pick = rng.integers(0, full.nnz, size=min(200, full.nnz))
        got = np.array([L.kmdbh_metric(names.index(name), int(full.val[e]), int(cnt[rows[e]]), int(cnt[full.col[e]]), k) for e in pick])
        assert np.array_equal(got, want[pick], equal_nan=True), name
    cases = []
    for name in names:
        vals = _np_metric(name, full.val, cnt[rows], cnt[full.col], k)
        fin = np.sort(vals[np.isfinite(vals)])
        if fin.size == 0:
            continue
        q = [float(fin[int(x * (fin.size - 1))]) for x in (0.0, 0.25, 0.5, 0.9, 1.0)]
        cases += [[(name, q[1], q[3])], [(name, q[2], None)], [(name, None, q[2])], [(name, q[2], q[2])], [(name, q[4] + 1.0, None)], [(name, None, None)]]
        other = names[(names.index(name) + 3) % len(names)]
        ov = _np_metric(other, full.val, cnt[rows], cnt[full.col], k)
        of = np.sort(ov[np.isfinite(ov)])
        cases.append([(name, q[1], None), (other, None, float(of[int(0.8 * (of.size - 1))]))])
    for ci, filters in enumerate(cases):
        keep = np.ones(full.nnz, dtype=bool)
        for name, lo, hi in filters:
            x = _np_metric(name, full.val, cnt[rows], cnt[full.col], k)
            with np.errstate(invalid="ignore"):
                keep &= (x >= (-np.finfo(np.float64).max if lo is None else lo)) & (x <= (np.finfo(np.float64).max if hi is None else hi))
        measure = names[ci % len(names)]
        sp = d.all2all_sparse_filtered(filters, cnt, measure=measure)
        assert sp.nnz == int(keep.sum()), (filters, sp.nnz, int(keep.sum()))
        assert np.array_equal(sp.col, full.col[keep]) and np.array_equal(sp.val, full.val[keep])
        assert np.array_equal(np.diff(sp.row_ptr), np.bincount(rows[keep], minlength=d.N))
        assert np.array_equal(sp.measure, _np_metric(measure, full.val, cnt[rows], cnt[full.col], k)[keep], equal_nan=True)


@pytest.mark.parametrize("stem", ["virus_k18", "synth_k21", "clade64", "clade64_k25_f01"])
def test_all2all_sparse_bit_exact(K, O, golden_dir, dev, stem):
    path = os.path.join(golden_dir, stem + ".db")
    d = K.DeviceDB(K.HostDB(path, skip_hashtables=True), device=dev)
    sp = d.all2all_sparse()
    flat = O.OracleDB(path, skip_hashtables=True).all2all_flat()
    lines = open(os.path.join(golden_dir, stem + ".a2a_sp.ref.txt"), "rb").read().split(b"\n")
    assert sp.n_rows == d.N
    for i in range(d.N):
        c, v = sp.row(i)
        row = O.tri_row(flat, i)
        nz = np.nonzero(row)[0]
        assert np.array_equal(c, nz) and np.array_equal(v, row[nz])
        assert "".join("%d:%d," % (a + 1, b) for a, b in zip(c, v)).encode() == lines[i]


@pytest.mark.parametrize("N,cs,L,r1,width", [(3000, 50, 1500, 0.75, 0), (2500, 40, 1200, 0.75, 64), (1200, 50, 3000, 0.10, 0)])
def test_all2all_sparse_scans_the_tiles_the_call_added_to(K, O, dev, tmp_path, N, cs, L, r1, width):
    """all2all-sp on data that is sparse (reference all2all_sp is O(nnz): src/similarity_calculator.cpp:596-638, src/array.h:391-446): clades
    from independent roots (r1 = 0.75) share nothing, only the blocks on the diagonal are non-zero.  The compaction scans the tiles the
    apply kernels flagged (kmdb_db.tile_touched) instead of all N (N - 1) / 2 cells: rows == the reference's all2all_sp text (or the
    oracle's matrix), == the scan of every cell (KMDB_SP_ALL_TILES=1), with bounds too, and with a block width that cuts the clades."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    device = torch.device("cuda", dev)
    g, pat = S.synth_database(N, cs, L, k=25, fraction=0.2, seed=41, r1=r1, device=device)
    arr = S.to_view_arrays(pat)
    path = str(tmp_path / "s.db")
    S.write_db_fast(path, 25, 0.2, [g.name(i) for i in range(N)], pat["sample_counts"], arr, device=device)
    exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
    view = K.make_view(25, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"])
    try:
        if width:
            os.environ["KMDB_BLOCK_WIDTH"] = str(width)
        d = K.DeviceDB(view, device=dev)
        sp = d.all2all_sparse()
        assert d.stats()["path"] == K.capi.PATH_RECORDS
        nz = np.nonzero(exp)[0]
        assert sp.nnz == nz.size and np.array_equal(sp.val, exp[nz])
        rr = np.repeat(np.arange(N, dtype=np.int64), np.diff(sp.row_ptr).astype(np.int64))
        assert np.array_equal(rr * (rr - 1) // 2 + sp.col.astype(np.int64), nz)
        if r1 > 0.5:
            assert sp.nnz < N * cs            # nothing outside the clades' own blocks
        if O.have_ref():
            txt, _ = O.ref_all2all_sp(path, str(tmp_path / "sp.txt"), threads=8)
            lines = txt.split(b"\n")
            for i in range(0, N, 7):
                c, v = sp.row(i)
                assert "".join("%d:%d," % (a + 1, b) for a, b in zip(c, v)).encode() == lines[i], i
        cnt = np.asarray(pat["sample_counts"], dtype=np.uint32)
        flt = [("jaccard", 0.3, None), ("num-kmers", 3.0, None)]
        a = d.all2all_sparse_filtered(flt, cnt, measure="ani")
        os.environ["KMDB_SP_ALL_TILES"] = "1"
        sp2 = d.all2all_sparse()
        b = d.all2all_sparse_filtered(flt, cnt, measure="ani")
        assert sp2.nnz == sp.nnz and np.array_equal(sp2.row_ptr, sp.row_ptr) and np.array_equal(sp2.col, sp.col) and np.array_equal(sp2.val, sp.val)
        assert a.nnz == b.nnz and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
        assert np.array_equal(a.measure, b.measure, equal_nan=True) and 0 < a.nnz < sp.nnz
        d.close()
    finally:
        os.environ.pop("KMDB_BLOCK_WIDTH", None)
        os.environ.pop("KMDB_SP_ALL_TILES", None)


def test_new2all_bit_exact(K, O, golden_dir, dev):
    path = os.path.join(golden_dir, "clade64.db")
    d = K.DeviceDB(K.HostDB(path), device=dev, with_hashtables=True)
    q = np.load(os.path.join(golden_dir, "clade64.queries.npz"))
    qs = [K.sort_unique(q[k]) for k in sorted(q.files, key=lambda s: int(s[1:]))]
    # plus edge cases: an empty query, k-mers absent from the db, a single k-mer
    qs += [np.zeros(0, np.uint64), np.array([1, 2, 3, (255 << 32) | 12345], np.uint64), qs[0][:1]]
    got = d.new2all(qs)
    o = O.OracleDB(path)
    exp = np.stack([o.one2all(x) for x in qs])
    assert np.array_equal(got, exp)
    ref = np.fromfile(os.path.join(golden_dir, "clade64.n2a.ref.u32"), dtype=np.uint32).reshape(-1, d.N)
    assert np.array_equal(got[: ref.shape[0]], ref)
    sp = d.new2all_sparse(qs)
    for i in range(len(qs)):
        c, v = sp.row(i)
        nz = np.nonzero(exp[i])[0]
        assert np.array_equal(c, nz) and np.array_equal(v, exp[i][nz])
    with pytest.raises(K.KmdbError, match="without hashtables"):
        K.DeviceDB(K.HostDB(path, skip_hashtables=True), device=dev).new2all(qs[:1])


def _virus_texts(golden_dir, list_name, limit):
    """sequence text of the genomes of a sample list: the records of one file joined by a newline"""
    texts = []
    with open(os.path.join(golden_dir, list_name)) as f:
        entries = [ln.strip() for ln in f if ln.strip()]
    for e in entries[:limit]:
        raw = open(os.path.join(golden_dir, e + ".fasta")).read()
        recs = [r.split("\n", 1)[1] if "\n" in r else "" for r in raw.split(">") if r]
        texts.append("\n".join(r.replace("\n", "").replace("\r", "") for r in recs))
    return texts


@pytest.mark.parametrize("stem,k,fraction", [("virus_k18_part1", 18, 1.0), ("virus_k25_f01_part1", 25, 0.1)])
def test_new2all_device_side_kmer_extraction(K, O, golden_dir, dev, stem, k, fraction):
    """kmdb_new2all_batch_seq (extraction + minhash filter + sort/unique on the device) against the host loader
    (kmdbh_extract_kmers + kmdbh_sort_unique = the reference's loader, pinned by the CLI goldens) and the oracle."""
    path = os.path.join(golden_dir, stem + ".db")
    d = K.DeviceDB(K.HostDB(path), device=dev, with_hashtables=True)
    texts = _virus_texts(golden_dir, "virus.seqs.part2.list", 12)
    # edge cases: lower case + U, an invalid symbol inside, shorter than k, empty, a record boundary right at a window
    texts += [texts[0].lower().replace("t", "u"), texts[1][:500] + "N" + texts[1][500:], "ACGT", "", "A" * (k - 1) + "\n" + "C" * (k - 1)]
    host = []
    for t in texts:
        parts = [K.extract_kmers(rec, k, fraction) for rec in t.split("\n")] if t else []
        host.append(K.sort_unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64))
    got, cnt = d.new2all_seq(texts, fraction=fraction)
    assert [int(c) for c in cnt] == [h.size for h in host]
    exp = d.new2all(host)
    assert np.array_equal(got, exp)
    o = O.OracleDB(path)
    assert np.array_equal(got[:3], np.stack([o.one2all(h) for h in host[:3]]))
    assert cnt[-1] == 0 and cnt[-2] == 0 and not got[-1].any()


@pytest.mark.parametrize("stem,k,alphabet", [("protein_aa", 8, "aa"), ("protein_aa11_diamond", 8, "aa11_diamond"), ("protein_aa12_mmseqs", 8, "aa12_mmseqs"),
                                              ("protein_aa6_dayhoff", 8, "aa6_dayhoff"), ("protein_aa_k7", 7, "aa")])
def test_new2all_on_the_protein_alphabets(K, O, golden_dir, dev, tmp_path, stem, k, alphabet):
    """new2all / one2all against the reference's test/protein databases (amino-acid alphabets of src/alphabet.h:79-126, n-bit symbols,
    strand preserved, src/kmer_extract.h:13-97): the records of aa_100x1000.fasta as queries through the query loader on the DEVICE
    (kmdb_new2all_batch_seq_alphabet) == the oracle's one2all of the oracle-extracted k-mers == the host loader's k-mers through
    kmdb_new2all_batch; a query that is a sample of the database finds all its k-mers in its own column; and the front-end's one2all
    runs on such a database (missing 4)."""
    import lzma
    path = os.path.join(golden_dir, stem + ".db")
    h = K.HostDB(path)
    assert K.ALPHABETS[h.alphabet] == alphabet
    d = K.DeviceDB(h, device=dev, with_hashtables=True)
    with lzma.open(os.path.join(ROOT, "tests", "golden", "protein.aa_100x1000.fasta.xz")) as f:
        recs = O._split_records(f.read())
    texts = [s for _, s in recs[:24]]
    # edge cases: lower case, a letter outside the alphabet inside, two records of one sample, shorter than k, empty
    texts += [texts[0].lower(), texts[1][:200] + b"X" + texts[1][200:], texts[2] + b"\n" + texts[3], b"ACDEF", b""]
    want = [O.sort_unique(np.concatenate([O.extract_seq_alphabet(r, k, alphabet) for r in t.split(b"\n")])) if t else np.zeros(0, np.uint64) for t in texts]
    got, cnt = d.new2all_seq(texts, alphabet=h.alphabet)
    assert [int(c) for c in cnt] == [w.size for w in want]
    o = O.OracleDB(path)
    assert np.array_equal(got, np.stack([o.one2all(w) for w in want]))
    host = [K.sort_unique(np.concatenate([K.extract_kmers_alphabet(r, k, h.alphabet) for r in t.split(b"\n")])) if t else np.zeros(0, np.uint64) for t in texts]
    assert all(np.array_equal(a, b) for a, b in zip(host, want)) and np.array_equal(d.new2all(host), got)
    for i in range(24):                                         # the database's samples are these records, in order
        assert got[i, i] == want[i].size
    assert not got[-1].any() and not got[-2].any()
    # the front-end: one2all of a record that is a sample — its row of the all2all golden, its own column = its k-mer count
    fa = tmp_path / "q.fasta"
    fa.write_bytes(b">q\n" + texts[5] + b"\n")
    out = tmp_path / "o.csv"
    _cli("one2all", path, str(fa), str(out))
    row = out.read_text().split("\n")[2].split(",")
    assert int(row[1]) == want[5].size and [int(x) for x in row[2:] if x] == [int(x) for x in got[5]]


def test_db2db_bit_exact(K, O, golden_dir, dev):
    """kmdb_db2db_dense (db2db_sp, the off-diagonal cell of all2all-parts) against the oracle, whose db2db is pinned to
    the reference's all2all matrix of the union database (tests/test_oracle_golden.py)."""
    p1, p2 = os.path.join(golden_dir, "virus_k18_part1.db"), os.path.join(golden_dir, "virus_k18_part2.db")
    d1 = K.DeviceDB(K.HostDB(p1), device=dev, with_hashtables=True)
    d2 = K.DeviceDB(K.HostDB(p2), device=dev, with_hashtables=True)
    o1, o2 = O.OracleDB(p1), O.OracleDB(p2)
    got = d2.db2db(d1)
    assert got.shape == (65, 100) and np.array_equal(got, o2.db2db(o1))
    assert np.array_equal(d1.db2db(d2), got.T)
    # a database against itself: the diagonal holds the samples' k-mer counts, the rest is the all2all matrix
    self_m = d1.db2db(d1)
    ref = np.fromfile(os.path.join(golden_dir, "virus_k18_part1.a2a.ref.u32"), dtype=np.uint32)
    for i in (1, 17, 99):
        assert np.array_equal(self_m[i, :i], O.tri_row(ref, i))
    h1 = K.HostDB(p1)
    assert [int(self_m[i, i]) for i in range(5)] == [int(K.capi.lib().kmdbh_db_sample_kmers(h1._h, i)) for i in range(5)]
    with pytest.raises(K.KmdbError, match="hashtables"):
        d1.db2db(K.DeviceDB(K.HostDB(p2, skip_hashtables=True), device=dev))
    with pytest.raises(K.KmdbError, match="k-mer lengths"):
        d1.db2db(K.DeviceDB(K.HostDB(os.path.join(golden_dir, "virus_k25_f01_part1.db")), device=dev, with_hashtables=True))


@pytest.mark.parametrize("N,L,near", [(5200, 1500, True), (9000, 400, False)])
def test_db2db_large_parts(K, O, dev, tmp_path, N, L, near):
    """db2db beyond round 1's limits.  near: near-identical genomes, patterns that list more samples than any fixed per-pattern
    buffer (round 1 refused > 2048); every row of the cell equals the corresponding part of the all2all matrix of the whole
    collection.  Otherwise: 4500 x 4500 samples = 71 x 71 block pairs, more than the one-pass counting sort takes (radix sort
    path of kmdb_rect_sort_apply), against the oracle."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    cs, k = 50, 18
    device = torch.device("cuda", dev)
    g = S.CladeGenomes(N, cs, L, r1=0.005 if near else 0.10, r2=0.0005 if near else 0.01, seed=11, device=device)
    ids_a, ids_b = list(range(0, N, 2)), list(range(1, N, 2))
    pa, pb, pall = str(tmp_path / "a.db"), str(tmp_path / "b.db"), str(tmp_path / "all.db")
    _synth_part(S, g, ids_a, k, pa, device)
    _synth_part(S, g, ids_b, k, pb, device)
    ha = K.HostDB(pa)
    da = K.DeviceDB(ha, device=dev, with_hashtables=True)
    db_ = K.DeviceDB(K.HostDB(pb), device=dev, with_hashtables=True)
    got = db_.db2db(da)
    if near:
        assert int(ha.view_arrays()["num_samples"].max()) > 2048          # the case this test is about
        _synth_part(S, g, ids_a + ids_b, k, pall, device)
        full = K.DeviceDB(K.HostDB(pall, skip_hashtables=True), device=dev).all2all_dense()
        na = len(ids_a)
        for r in range(0, len(ids_b), 97):
            assert np.array_equal(got[r], O.tri_row(full, na + r)[:na]), r
        # and straight from the definition: shared k-mers of the two samples' k-mer sets (no pattern, no tree involved)
        ka = [S.kmers_of(g.sample(i), k) for i in ids_a[:: max(1, len(ids_a) // 11)]]
        for r in (0, 1, len(ids_b) // 2, len(ids_b) - 1):
            kb = S.kmers_of(g.sample(ids_b[r]), k)
            want = [int(torch.isin(kb, x).sum()) for x in ka]
            assert got[r][:: max(1, len(ids_a) // 11)][: len(want)].tolist() == want, r
    else:
        assert np.array_equal(got, O.OracleDB(pb).db2db(O.OracleDB(pa))) and got.any()
    assert np.array_equal(da.db2db(db_), got.T)


SAMPLE_ROWS = [("virus_k18", "sr_jaccard5", ["-sample-rows", "jaccard:5"]), ("virus_k18", "sr_numkmers3_min", ["-sample-rows", "num-kmers:3", "-min", "jaccard:0.02"]),
               ("clade64", "sr_ani7", ["-sample-rows", "ani:7"]), ("clade64", "sr_max2", ["-sample-rows", "max:2", "-max", "num-kmers:3000"])]


def test_sample_rows_like_the_reference(golden_dir, dev, tmp_path):
    """`-sample-rows [<criterion>:]<count>` of all2all-sp and all2all-parts (reference src/sampler.h, src/params.cpp:533-557, src/array.h:450-540;
    SURVEY 2 #9: the front-end must honour it; VERDICT round 5, missing 5).  With a criterion the rows — symmetric: a pair is offered to both its
    samples — are the reference's byte for byte: tests/golden/*.sr_*.ref.txt were written by the reference's own Sampler (make_fixture_sample_rows.py),
    and where oracle/_ref travels the reference runs again beside the front-end.  all2all-parts -sample-rows over the two virus parts gives the same
    rows as all2all-sp over the whole collection.  Random strategy (no criterion): at most `count` valid pairs per row, a pair listed by either of
    its samples was a pair of the unsampled output (the subset itself depends on the reference's hash-table order and is not compared)."""
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    exe = os.path.join(ROOT, "oracle", "_ref", "bridge_driver")

    def rows_of(csv):
        return [b",".join(ln.split(b",")[2:]) for ln in open(csv, "rb").read().split(b"\n")[2:] if ln]

    for stem, tag, opts in SAMPLE_ROWS:
        _cli("all2all-sp", *opts, g(stem + ".db"), t(tag + ".csv"))
        want = open(g("%s.%s.ref.txt" % (stem, tag)), "rb").read().split(b"\n")[:-1]
        assert rows_of(t(tag + ".csv")) == want, tag
        if os.path.exists(exe):
            r = subprocess.run([exe, "sample_rows_ref", g(stem + ".db"), t(tag + ".ref")] + opts, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert open(t(tag + ".ref"), "rb").read().split(b"\n")[:-1] == want
    # the whole file has the shape of the unsampled one: header, counts, name + k-mer count in front of every row
    plain = t("plain.csv")
    _cli("all2all-sp", g("virus_k18.db"), plain)
    a, b = open(plain, "rb").read().split(b"\n"), open(t("sr_jaccard5.csv"), "rb").read().split(b"\n")
    assert a[:2] == b[:2] and [x.split(b",")[:2] for x in a[2:]] == [x.split(b",")[:2] for x in b[2:]]
    # all2all-parts: the same rows from the grid of cells
    with open(t("db.list"), "w") as f:
        f.write(g("virus_k18_part1.db") + "\n" + g("virus_k18_part2.db") + "\n")
    for extra in ([], ["-gpus", "2"]):
        _cli("all2all-parts", "-sample-rows", "jaccard:5", *extra, t("db.list"), t("parts.csv"))
        assert rows_of(t("parts.csv")) == open(g("virus_k18.sr_jaccard5.ref.txt"), "rb").read().split(b"\n")[:-1]
    # random strategy
    _cli("all2all-sp", "-sample-rows", "4", g("clade64.db"), t("rnd.csv"))
    _cli("all2all-sp", g("clade64.db"), t("clade.csv"))
    pairs = set()
    for i, row in enumerate(rows_of(t("clade.csv"))):
        for cell in row.split(b",")[:-1]:
            c, v = cell.split(b":")
            pairs.add((i, int(c) - 1, int(v)))
    for i, row in enumerate(rows_of(t("rnd.csv"))):
        cells = [c.split(b":") for c in row.split(b",")[:-1]]
        ids = [int(c) - 1 for c, _ in cells]
        assert len(cells) <= 4 and ids == sorted(set(ids))
        for c, v in cells:
            j = int(c) - 1
            assert (max(i, j), min(i, j), int(v)) in pairs


def test_all2all_parts_grid_over_the_devices_of_a_node(K, O, dev, tmp_path):
    """`kmer-db-amd all2all-parts -gpus W` (the grid of cells over the GPUs; reference src/console_all2all_parts.cpp:143-331 walks it
    on one CPU): a collection in FIVE part databases, block rows dealt to 1 / 2 / 3 / 5 workers (on this box they share the one GPU, every worker
    with its own resident parts) — the outputs are byte-identical, and equal to the sparse all2all of the whole collection (all2all-sp CLI)."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    N, cs, L, k = 150, 25, 5000, 18
    device = torch.device("cuda", dev)
    g = S.CladeGenomes(N, cs, L, seed=17, device=device)
    cuts = [0, 20, 55, 90, 101, N]                               # (parts of unequal size; sample order = the collection's)
    paths = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        paths.append(str(tmp_path / ("p%d.db" % a)))
        _synth_part(S, g, list(range(a, b)), k, paths[-1], device)
    pall = str(tmp_path / "all.db")
    _synth_part(S, g, list(range(N)), k, pall, device)
    lst = tmp_path / "parts.list"
    lst.write_text("".join(p + "\n" for p in paths))
    outs = {}
    for w in (None, "2", "3", "5"):
        out = str(tmp_path / ("parts_%s.csv" % w))
        _cli("all2all-parts", *(["-gpus", w] if w else []), str(lst), out)
        outs[w] = open(out, "rb").read()
    assert outs[None] == outs["2"] == outs["3"] == outs["5"] and outs[None].count(b"\n") == N + 2
    whole = str(tmp_path / "whole.csv")
    _cli("all2all-sp", pall, whole)
    assert open(whole, "rb").read() == outs[None]


def test_db2db_with_more_than_65535_samples(K, O, dev, tmp_path):
    """all2all-parts with a part of 66 000 samples (reference: 32-bit sample ids, src/types.h:15-18; src/console_all2all_parts.cpp:159-226): round
    4's pair kernel kept its block indices in a fixed 1024-entry LDS array and refused.  Two pattern forests with fabricated k-mer
    dictionaries that overlap in part (db2db looks k-mers up, it never extracts them), both directions against the oracle."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    rng = np.random.default_rng(660)
    k = 18

    def part(N, P, max_local, pool, n_kmers, path):
        pat = _random_forest(rng, N, P, max_local, chain_frac=0.4)
        pids = np.sort(rng.integers(1, P, size=n_kmers))
        pat["num_kmers"] = torch.from_numpy(np.bincount(pids, minlength=P).astype(np.int64))
        kmers = np.sort(pool[:n_kmers])
        arr = S.to_view_arrays(pat)
        tables = S.build_hashtables(torch.from_numpy(kmers.astype(np.int64)), torch.from_numpy(rng.permutation(pids).astype(np.int64)), k)
        S.write_db(path, k, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr, kmers_count=n_kmers, tables=tables)
        return K.DeviceDB(K.HostDB(path), device=dev, with_hashtables=True), O.OracleDB(path)

    universe = rng.choice(1 << 36, size=9000, replace=False).astype(np.uint64)
    pa, pb = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    da, oa = part(66000, 2500, 400, universe, 6000, pa)                      # k-mers universe[0 .. 6000)
    db_, ob = part(700, 600, 60, universe[3000:], 5000, pb)                  # k-mers universe[3000 .. 8000): 3000 shared
    assert int(da.N) == 66000
    got = db_.db2db(da)
    exp = ob.db2db(oa)
    assert got.shape == (700, 66000) and np.array_equal(got, exp) and got[:, 65536:].any() and got.any()
    assert np.array_equal(da.db2db(db_), exp.T)


def _synth_part(S, g, ids, k, path, device):
    """database (with hashtables) of the samples `ids` of the genome model g, written in kmer-db's format"""
    pat = S.build_patterns(lambda i: S.kmers_of(g.sample(ids[i]), k), len(ids), device)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    S.write_db(path, k, 1.0, [g.name(i) for i in ids], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)


@pytest.mark.parametrize("split", ["halves", "interleaved"])
def test_db2db_synthetic_parts(K, O, dev, tmp_path, split, monkeypatch):
    """db2db on two parts of one clade-structured collection: GPU == oracle == the real reference's db2db_sp, and the
    cell equals the corresponding block of the all2all matrix of the whole collection."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    N, cs, L, k = 120, 20, 6000, 18
    device = torch.device("cuda", dev)
    g = S.CladeGenomes(N, cs, L, seed=5, device=device)
    ids_a = list(range(N // 2)) if split == "halves" else list(range(0, N, 2))
    ids_b = list(range(N // 2, N)) if split == "halves" else list(range(1, N, 2))
    pa, pb, pall = str(tmp_path / "a.db"), str(tmp_path / "b.db"), str(tmp_path / "all.db")
    _synth_part(S, g, ids_a, k, pa, device)
    _synth_part(S, g, ids_b, k, pb, device)
    _synth_part(S, g, ids_a + ids_b, k, pall, device)
    da = K.DeviceDB(K.HostDB(pa), device=dev, with_hashtables=True)
    db_ = K.DeviceDB(K.HostDB(pb), device=dev, with_hashtables=True)
    bytes0 = da.stats()["device_bytes"]
    got = db_.db2db(da)
    exp = O.OracleDB(pb).db2db(O.OracleDB(pa))
    assert np.array_equal(got, exp) and got.any()
    # the call left the patterns' full lists with both handles (db2db.hip, list store); handles that do without it
    # (as parts of more than 4096 samples do) climb the root paths and give the same cell
    assert da.stats()["device_bytes"] > bytes0
    assert np.array_equal(db_.db2db(da), got)
    monkeypatch.setenv("KMDB_D2_NO_STORE", "1")
    da2 = K.DeviceDB(K.HostDB(pa), device=dev, with_hashtables=True)
    db2 = K.DeviceDB(K.HostDB(pb), device=dev, with_hashtables=True)
    bytes2 = da2.stats()["device_bytes"]
    assert np.array_equal(db2.db2db(da2), got) and da2.stats()["device_bytes"] == bytes2
    monkeypatch.delenv("KMDB_D2_NO_STORE")
    full = K.DeviceDB(K.HostDB(pall, skip_hashtables=True), device=dev).all2all_dense()
    na = len(ids_a)
    for r in (0, 7, len(ids_b) - 1):
        assert np.array_equal(got[r], O.tri_row(full, na + r)[:na])
    if O.have_ref():
        txt, _ = O.ref_db2db_sp(pb, pa, str(tmp_path / "ref.txt"), threads=2)
        lines = txt.split(b"\n")
        for r in range(len(ids_b)):
            assert "".join("%d:%d," % (c + 1, v) for c, v in enumerate(got[r]) if v).encode() == lines[r]


def _cli(*args):
    exe = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def _same(a, b):
    assert open(a, "rb").read() == open(b, "rb").read(), (a, b)


def test_cli_byte_identical_to_reference_goldens(golden_dir, dev, tmp_path):
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    # .github/workflows/main.yml:87-95 / 110-114 / 135-152
    _cli("all2all", g("virus_k18_parts.db"), t("k18.csv")); _same(t("k18.csv"), g("virus.k18.csv"))
    _cli("all2all", "-sparse", g("virus_k18_parts.db"), t("k18.sparse.csv")); _same(t("k18.sparse.csv"), g("virus.k18.sparse.csv"))
    _cli("all2all-sp", g("virus_k18.db"), t("k18.sp.csv")); _same(t("k18.sp.csv"), g("virus.k18.sparse.csv"))
    _cli("all2all", "-t", "2", g("virus_k18_f01.db"), t("frac.csv")); _same(t("frac.csv"), g("virus.k18.frac.csv"))
    _cli("all2all", g("virus_k24.db"), t("k24.csv")); _same(t("k24.csv"), g("virus.k24.csv"))
    # the same through the multi-GPU driver of the front-end (kmdb_node_*): N prefix-bucket shards over the devices of the box — on a one-GPU
    # box the shards of the device run one after the other and are summed on the device; with more devices RCCL reduce-scatters
    r = _cli("all2all", "-gpus", "2", g("virus_k18_parts.db"), t("k18.g2.csv")); _same(t("k18.g2.csv"), g("virus.k18.csv"))
    assert "2 shards on" in r.stderr
    _cli("all2all", "-sparse", "-gpus", "5", g("virus_k18_parts.db"), t("k18.g5.sparse.csv")); _same(t("k18.g5.sparse.csv"), g("virus.k18.sparse.csv"))
    _cli("all2all-sp", "-gpus", "3", g("virus_k18.db"), t("k18.sp.g3.csv")); _same(t("k18.sp.g3.csv"), g("virus.k18.sparse.csv"))
    _cli("all2all", "-gpus", "1", g("virus_k24.db"), t("k24.g1.csv")); _same(t("k24.g1.csv"), g("virus.k24.csv"))
    _cli("all2all-sp", "-gpus", "4", "-max", "39", "-min", "num-kmers:31", g("synth_k21.db"), t("a2a-sp-mm.g4")); _same(t("a2a-sp-mm.g4"), g("synth.a2a.sparse.above-below"))
    # self-hosted.yml:393-403 (test/protein: DNA records as samples, k = 24, canonical and strand-preserving k-mers)
    _cli("all2all", g("protein_dna_k24.db"), t("dna.a2a")); _same(t("dna.a2a"), g("protein.dna.a2a"))
    _cli("all2all", g("protein_dna_k24_preserve.db"), t("dna-p.a2a")); _same(t("dna-p.a2a"), g("protein.dna-preserve.a2a"))
    _cli("all2all", "-gpus", "3", g("protein_dna_k24_preserve.db"), t("dna-p3.a2a")); _same(t("dna-p3.a2a"), g("protein.dna-preserve.a2a"))
    # self-hosted.yml:404-427 (test/protein: amino-acid alphabets, k = 8; aa_k7.a2a at k = 7) — all2all never looks at the alphabet
    for stem in ("aa", "aa11_diamond", "aa12_mmseqs", "aa6_dayhoff", "aa_k7"):
        _cli("all2all", g("protein_%s.db" % stem), t(stem + ".a2a")); _same(t(stem + ".a2a"), g("protein.%s.a2a" % stem))
    # self-hosted.yml:110-146 (synth, with min/max filters)
    _cli("all2all", g("synth_k21.db"), t("a2a")); _same(t("a2a"), g("synth.a2a"))
    _cli("all2all", "-sparse", g("synth_k21.db"), t("a2a-sparse")); _same(t("a2a-sparse"), g("synth.a2a-sparse"))
    _cli("all2all", "-sparse", "-max", "39", "-min", "num-kmers:31", g("synth_k21.db"), t("a2a-mm")); _same(t("a2a-mm"), g("synth.a2a.sparse.above-below"))
    _cli("all2all-sp", g("synth_k21.db"), t("a2a-sp")); _same(t("a2a-sp"), g("synth.a2a-sparse"))
    _cli("all2all-sp", "-max", "39", "-min", "num-kmers:31", g("synth_k21.db"), t("a2a-sp-mm")); _same(t("a2a-sp-mm"), g("synth.a2a.sparse.above-below"))
    # new2all: main.yml:73-81, 160-163; self-hosted.yml:188-201
    cwd = os.getcwd()
    os.chdir(golden_dir)          # list entries are ./test/virus/data/<name>
    try:
        _cli("new2all", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("n2a.csv")); _same(t("n2a.csv"), g("virus.k18.n2a.csv"))
        _cli("new2all", "-sparse", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("n2a.sp.csv")); _same(t("n2a.sp.csv"), g("virus.k18.n2a.sparse.csv"))
        _cli("new2all", g("virus_k18.db"), g("virus.seqs.list"), t("n2a.it.csv")); _same(t("n2a.it.csv"), g("virus.k18.n2a.itself.csv"))
        # the same with the loader on the host (-host-extract): kmdb_new2all_batch instead of kmdb_new2all_batch_seq
        _cli("new2all", "-host-extract", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("n2a.h.csv")); _same(t("n2a.h.csv"), g("virus.k18.n2a.csv"))
        with open(t("synth.list"), "w") as f:
            f.write(g("synth.synth") + "\n")
        _cli("new2all", "-multisample-fasta", g("synth_k21.db"), t("synth.list"), t("n2a")); _same(t("n2a"), g("synth.n2a"))
        _cli("new2all", "-multisample-fasta", "-sparse", g("synth_k21.db"), t("synth.list"), t("n2a-sp")); _same(t("n2a-sp"), g("synth.n2a-sparse"))
        _cli("new2all", "-multisample-fasta", "-sparse", "-max", "69", "-min", "num-kmers:21", g("synth_k21.db"), t("synth.list"), t("n2a-mm"))
        _same(t("n2a-mm"), g("synth.n2a.sparse.above-below"))
        # all2all-parts: self-hosted.yml:355-362 (two part databases, output = sparse all2all of the whole collection)
        with open(t("db.list"), "w") as f:
            f.write(g("virus_k18_part1.db") + "\n" + g("virus_k18_part2.db") + "\n")
        _cli("all2all-parts", t("db.list"), t("k18.parts.csv")); _same(t("k18.parts.csv"), g("virus.k18.sparse.csv"))
        # the block rows of the grid dealt to workers over the node's devices (-gpus W; on this box they share the one GPU), rows written in order
        for w in ("2", "3"):
            _cli("all2all-parts", "-gpus", w, t("db.list"), t("k18.parts%s.csv" % w)); _same(t("k18.parts%s.csv" % w), g("virus.k18.sparse.csv"))
        # one2all: main.yml:156-160 (k=25, f=0.1 database of part 1, one genome against it)
        _cli("one2all", g("virus_k25_f01_part1.db"), "./test/virus/data/MT159713", t("MT159713.csv"))
        _same(t("MT159713.csv"), g("virus.MT159713.csv"))
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("N,cs,L,k", [(1000, 50, 30000, 18), (1500, 30, 6000, 18), (300, 300, 20000, 18), (2048, 64, 3000, 18)])
def test_synthetic_databases_bit_exact(K, O, dev, tmp_path, N, cs, L, k):
    """Bench-shaped inputs (BASELINE.json configs[1] at reduced genome length), generated on the GPU,
    run through every all2all kernel and compared with the oracle (and the real reference when
    oracle/_ref travelled with the snapshot)."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    g, pat = S.synth_database(N, cs, L, k=k, seed=3, device=torch.device("cuda", dev))
    arr = S.to_view_arrays(pat)
    path = str(tmp_path / "s.db")
    S.write_db(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr)
    exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
    if O.have_ref():
        mr, _ = O.ref_all2all(path, str(tmp_path / "m.u32"), threads=8)
        assert np.array_equal(mr, exp)
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    got = d.all2all_dense()
    assert np.array_equal(got, exp)
    st = d.stats()
    assert st["n_records"] > 0 and st["path"] == K.capi.PATH_RECORDS and st["sum_pairs"] == int(exp.astype(np.uint64).sum())
    for fl in (K.capi.FLAG_FORCE_TILE, K.capi.FLAG_FORCE_GLOBAL_ATOMICS):
        assert np.array_equal(d.all2all_dense(flags=fl), exp), fl
    # the same database read back through the front-end's .db reader
    d2 = K.DeviceDB(K.HostDB(path, skip_hashtables=True), device=dev)
    assert np.array_equal(d2.all2all_dense(), exp)


@pytest.mark.parametrize("N,cs,L", [(3000, 100, 1500), (5000, 50, 600)])
def test_many_samples_on_the_block_record_pipeline(K, O, dev, tmp_path, N, cs, L):
    """The block-record pipeline has no sample-count limit (the reference has none either,
    similarity_calculator.cpp:42-438, array.h:136-140): thousands of samples = hundreds of blocks."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    g, pat = S.synth_database(N, cs, L, k=18, seed=9, device=torch.device("cuda", dev))
    arr = S.to_view_arrays(pat)
    path = str(tmp_path / "s.db")
    S.write_db(path, 18, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr)
    exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
    view = K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp)
    st = d.stats()
    assert st["path"] == K.capi.PATH_RECORDS and st["n_records"] > 0
    assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_FORCE_GLOBAL_ATOMICS), exp)
    sp = d.all2all_sparse()
    for i in (1, N // 2, N - 1):
        c, v = sp.row(i)
        row = O.tri_row(exp, i)
        nz = np.nonzero(row)[0]
        assert np.array_equal(c, nz) and np.array_equal(v, row[nz])


@pytest.mark.parametrize("stem,shards", [("virus_k18", 2), ("virus_k18", 8), ("clade64", 3), ("virus_k24", 5)])
def test_upload_shards_of_a_real_db_sum_to_full_matrix(K, golden_dir, dev, stem, shards):
    """kmdb_db_upload_shard on a .db built by the real reference: shard s keeps the k-mers of the prefix buckets b with
    b % shards == s (w_s[p] from the hashtable items, reference src/hashmap_lp.h:71-78, bucket = kmer >> 32 types.h:25-27);
    every shard runs the block-record pipeline and the partial matrices sum to the reference's matrix."""
    h = K.HostDB(os.path.join(golden_dir, stem + ".db"))
    ref = np.fromfile(os.path.join(golden_dir, stem + ".a2a.ref.u32"), dtype=np.uint32) if stem != "virus_k24" else \
        K.DeviceDB(h, device=dev).all2all_dense()
    acc = np.zeros_like(ref)
    total_pairs = 0
    kept = []
    for s in range(shards):
        d = K.DeviceDB(h, device=dev, prefix_shard=(s, shards))
        part = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
        st = d.stats()
        assert st["path"] == K.capi.PATH_RECORDS and (st["n_records"] > 0 or st["sum_pairs"] == 0)
        # the shard's tree: only the nodes whose subtree holds one of its k-mers (every k-mer sits in one shard, so the shards' trees
        # are proper parts of the whole one)
        assert 0 < st["n_patterns"] < d.P
        kept.append(st["n_patterns"])
        assert st["sum_pairs"] == int(part.astype(np.uint64).sum())          # the shard's own checksum identity
        total_pairs += st["sum_pairs"]
        acc += part
        d.close()
    assert np.array_equal(acc, ref) and total_pairs == int(ref.astype(np.uint64).sum())
    assert sum(kept) < shards * d.P                               # the front half of the pipeline is sharded too, not only the weights
    with pytest.raises(K.KmdbError, match="no hashtables"):
        K.DeviceDB(K.HostDB(os.path.join(golden_dir, stem + ".db"), skip_hashtables=True), device=dev, prefix_shard=(0, 2))


@pytest.mark.parametrize("stem,shards", [("virus_k18", 3), ("clade64", 8), ("clade64_k25_f01", 2)])
def test_node_driver_over_the_devices_of_the_box(K, golden_dir, dev, stem, shards):
    """kmdb_node_* (the C++ multi-GPU driver behind `kmer-db-amd all2all -gpus N`): shards over every device the box has (one here: the shards
    run in turn and are summed on the device; more: one RCCL reduce-scatter), dense matrix == the reference's, sparse rows (with bounds and a
    measure on the complete sums) == the single-device filtered call."""
    h = K.HostDB(os.path.join(golden_dir, stem + ".db"))
    ref = np.fromfile(os.path.join(golden_dir, stem + ".a2a.ref.u32"), dtype=np.uint32)
    devices = list(range(K.device_count()))
    nd = K.NodeDB(h, shards, devices)
    assert np.array_equal(nd.all2all_dense(), ref)
    st = nd.stats()
    assert st["n_shards"] == shards and st["n_devices"] == min(shards, len(devices)) and st["call_ms"] > 0
    assert (st["rccl_version"] > 0) == (st["n_devices"] > 1)
    assert np.array_equal(nd.all2all_dense(), ref)                    # warm call
    cnt = h.sample_kmers.astype(np.uint32)
    d1 = K.DeviceDB(h, device=dev)
    # every device by itself (kmdb_node_device_stats), and what crossed PCIe: a device receives the nodes its shards KEEP (planned on the
    # host for all shards at once) — their 24 bytes of header fields and their streams — and no hashtable slot.  The sum over the
    # devices is the sum of the kept nodes, not shards x the whole tree + all slots as in round 4.  (VERDICT round 4 asked for <= 1.3 x
    # the single-device upload; on these databases every pattern holds many k-mers, so nearly every shard keeps nearly every node —
    # sum(kept) is 1.5 - 6.4 x P, tests/test_host_cpu.py::test_shard_plan_on_the_host — and the bound is what the plan says, to the byte.)
    kept, kmers = h.shard_plan_counts(shards)
    one = d1.stats()["h2d_bytes"]
    assert one > 0 and len(st["devices"]) == st["n_devices"] and st["plan_s"] > 0
    assert sum(x["n_shards"] for x in st["devices"]) == shards
    assert sum(x["n_patterns"] for x in st["devices"]) == int(kept.sum())
    slots_bytes = 8 * int(h.view_arrays()["slots"].size)
    total = sum(x["h2d_bytes"] for x in st["devices"])
    stream_bytes = one - 32 * d1.P                                    # a whole upload: 24 B of fields + the 8-byte k-mer count per node, and the streams
    assert 24 * int(kept.sum()) < total <= 24 * int(kept.sum()) + shards * stream_bytes, (total, one, kept)
    assert total < shards * one and (shards * slots_bytes > total or slots_bytes == 0)
    for x in st["devices"]:
        assert x["call_ms"] > 0 and x["upload_s"] > 0 and x["n_records"] > 0 and x["h2d_bytes"] > 0
    a = d1.all2all_sparse()
    b = nd.all2all_sparse()
    assert a.nnz == b.nnz and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
    flt = [("jaccard", 0.02, None), ("num-kmers", None, 5000.0)]
    a = d1.all2all_sparse_filtered(flt, cnt, measure="mash")
    b = nd.all2all_sparse(flt, cnt, measure="mash")
    assert a.nnz == b.nnz and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
    assert np.array_equal(a.measure, b.measure, equal_nan=True)
    nd.close()
    d1.close()
    with pytest.raises(K.KmdbError, match="need the hashtables"):
        K.NodeDB(K.HostDB(os.path.join(golden_dir, stem + ".db"), skip_hashtables=True), 2, devices)
    with pytest.raises(K.KmdbError, match="listed twice"):
        K.NodeDB(h, 2, [0, 0])
    # the shards planned in rounds (the plan's weight counters held to a budget: here so small that every round holds as many shards as
    # there are devices) give the same handle
    os.environ["KMDB_PLAN_BUDGET_MB"] = "1"
    try:
        nd2 = K.NodeDB(h, shards, devices)
        assert np.array_equal(nd2.all2all_dense(), ref)
        assert sum(x["n_patterns"] for x in nd2.stats()["devices"]) == int(kept.sum())
        nd2.close()
    finally:
        del os.environ["KMDB_PLAN_BUDGET_MB"]
    with pytest.raises(K.KmdbError, match="shards"):
        K.NodeDB(h, 5000, devices)


def test_node_driver_rccl_calls_on_a_one_rank_communicator(K, golden_dir, dev, monkeypatch):
    """The RCCL half of kmdb_node_* on a one-GPU box: KMDB_NODE_FORCE_RCCL=1 makes the driver dlopen librccl, build its communicator with
    ncclCommInitAll and run the per-call ncclReduceScatter (uint32 sum, on the device's stream, events around it) on ONE rank — the same
    calls, arguments and ordering the multi-GPU run makes, minus the peers.  Three shards on the device are summed first; the chunk that
    comes out of the collective is the matrix (dense) or is compacted where it is (sparse)."""
    monkeypatch.setenv("KMDB_NODE_FORCE_RCCL", "1")
    h = K.HostDB(os.path.join(golden_dir, "virus_k18.db"))
    ref = np.fromfile(os.path.join(golden_dir, "virus_k18.a2a.ref.u32"), dtype=np.uint32)
    nd = K.NodeDB(h, 3, [dev])
    assert np.array_equal(nd.all2all_dense(), ref)
    st = nd.stats()
    assert st["n_devices"] == 1 and st["n_shards"] == 3 and st["rccl_version"] > 0 and st["collective_ms"] > 0
    assert np.array_equal(nd.all2all_dense(), ref)                    # warm call
    d1 = K.DeviceDB(h, device=dev)
    a, b = d1.all2all_sparse(), nd.all2all_sparse()
    assert a.nnz == b.nnz and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
    nd.close()
    d1.close()
    monkeypatch.delenv("KMDB_NODE_FORCE_RCCL")
    nd = K.NodeDB(h, 3, [dev])
    assert np.array_equal(nd.all2all_dense(), ref) and nd.stats()["rccl_version"] == 0        # without the switch one device needs no librccl
    nd.close()


@pytest.mark.parametrize("stem,shards", [("clade64_k25_f01", 2), ("virus_k18", 3), ("clade64", 8)])
def test_sharded_all2all_sp_from_the_reduced_matrix(K, golden_dir, dev, stem, shards):
    """BASELINE configs[3] on several GPUs, emulated on one: every prefix-bucket shard (kmdb_db_upload_shard) accumulates its partial
    matrix on the device, the partial matrices are summed (the RCCL reduce-scatter of bench.py --mode all2all-sp --gpus N), and every
    rank compacts ITS flat chunk of the triangle with kmdb_sparse_from_dense_device.  The ranks' rows, concatenated, are the reference's
    all2all_sp output (similarity_calculator.cpp:442-657 + array.h:391-446, console_all2all_sparse.cpp:44-96)."""
    import torch
    h = K.HostDB(os.path.join(golden_dir, stem + ".db"))
    N = h.N
    cells = N * (N - 1) // 2
    acc = torch.zeros(cells, dtype=torch.int32, device="cuda:%d" % dev)
    part = torch.empty_like(acc)
    d = None
    for s in range(shards):
        if d is not None:
            d.close()
        d = K.DeviceDB(h, device=dev, prefix_shard=(s, shards))
        d.all2all_dense_device(part.data_ptr())
        torch.cuda.synchronize()
        acc += part
    lines = open(os.path.join(golden_dir, stem + ".a2a_sp.ref.txt"), "rb").read().split(b"\n")
    per = (cells + shards - 1) // shards                              # reduce_scatter chunks: equal flat ranges of the triangle
    got = [b""] * N
    nnz = 0
    for r in range(shards):
        lo, hi = min(cells, r * per), min(cells, (r + 1) * per)
        chunk = acc[lo:hi].clone() if hi > lo else torch.zeros(1, dtype=torch.int32, device=acc.device)      # the rank's own buffer
        sp = d.sparse_from_dense_device(chunk.data_ptr(), lo, hi)
        assert sp.n_rows == N
        nnz += sp.nnz
        for i in range(N):
            c, v = sp.row(i)
            assert c.size == 0 or (lo <= i * (i - 1) // 2 + int(c[0]) and i * (i - 1) // 2 + int(c[-1]) < hi)
            got[i] += "".join("%d:%d," % (a + 1, b) for a, b in zip(c, v)).encode()
    for i in range(N):
        assert got[i] == lines[i], i
    full = d.sparse_from_dense_device(acc.data_ptr())
    assert full.nnz == nnz == int((acc != 0).sum().item())
    # bounds + measure on the reduced matrix == the single-GPU filtered call
    cnt = h.sample_kmers.astype(np.uint32)
    d1 = K.DeviceDB(h, device=dev)
    flt = [("jaccard", 0.02, None), ("num-kmers", None, 5000.0)]
    a = d1.all2all_sparse_filtered(flt, cnt, measure="mash")
    b = d.sparse_from_dense_device(acc.data_ptr(), filters=flt, sample_kmers=cnt, measure="mash")
    assert a.nnz == b.nnz and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
    assert np.array_equal(a.measure, b.measure, equal_nan=True)
    with pytest.raises(K.KmdbError, match="cell_lo > cell_hi"):
        d.sparse_from_dense_device(acc.data_ptr(), 10, 5)
    d.close()
    d1.close()


@pytest.mark.parametrize("N,cs,L,k,f,check", [(10000, 50, 400, 18, 1.0, "oracle"), (20000, 50, 700, 25, 0.1, "oracle"),
                                               (50000, 50, 1000, 25, 0.1, "checksum")])
def test_baseline_sample_counts_on_the_block_record_pipeline(K, O, dev, tmp_path, N, cs, L, k, f, check):
    """BASELINE.json configs [2]-[4] have 10 000 and 50 000 samples (k=18 f=1 / k=25 f=0.1): the same sample counts at
    genome lengths the oracle can afford, bit-exact; at 50 000 samples (5 GB matrix) through the checksum identity and
    the sparse entry point's structure."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    device = torch.device("cuda", dev)
    lap = _Laps("baseline_sample_counts[%d]" % N)
    g, pat = S.synth_database(N, cs, L, k=k, fraction=f, seed=11, device=device)
    arr = S.to_view_arrays(pat)
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    lap("database, upload")
    if check == "oracle":
        path = str(tmp_path / "s.db")
        S.write_db_fast(path, k, f, [g.name(i) for i in range(N)], pat["sample_counts"], arr, device=device)
        exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
        lap("file, oracle")
        got = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
        assert np.array_equal(got, exp)
        st = d.stats()
        assert st["path"] == K.capi.PATH_RECORDS and st["n_records"] > 0 and st["sum_pairs"] == int(exp.astype(np.uint64).sum())
        # and the same file read back by the front-end's reader
        assert np.array_equal(K.DeviceDB(K.HostDB(path, skip_hashtables=True), device=dev).all2all_dense(), exp)
        lap("calls, reader")
        Mrows = d.all2all_dense()
        row_cells = lambda i, cols: O.tri_row(Mrows, i)[cols]      # noqa: E731
    else:
        M = torch.zeros(d.tri_size(), dtype=torch.int32, device=device)
        d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_NO_FALLBACK)
        st = d.stats()
        assert st["path"] == K.capi.PATH_RECORDS and st["n_records"] > 0
        assert int(M.to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item()) == st["sum_pairs"]
        lap("call, checksum")
        # the sparse entry point over all 1.25 G cells, with a bound that leaves the pairs inside the clades (the unfiltered CSR of this
        # collection is 10 GB of host arrays: most cross-clade pairs share a k-mer or two): every kept cell equals the dense one, and
        # spot rows of the unfiltered compaction (kmdb_sparse_from_dense_device on the rows' own cells) list exactly the non-zero cells
        # (the 5 GB matrix stays on the device: the kept cells and the spot rows are fetched from it)
        cnt = np.asarray(pat["sample_counts"], dtype=np.uint32)
        sp = d.all2all_sparse_filtered([("num-kmers", 12.0, None)], cnt)
        assert sp.n_rows == N and 0 < sp.nnz < 200_000_000
        rr = np.repeat(np.arange(N, dtype=np.int64), np.diff(sp.row_ptr).astype(np.int64))
        at = torch.from_numpy(rr * (rr - 1) // 2 + sp.col.astype(np.int64)).to(device)
        assert np.array_equal(M[at].cpu().numpy().view(np.uint32), sp.val) and int(sp.val.min()) >= 12
        assert sp.nnz == int((M.view(torch.int32) >= 12).sum().item())
        del at
        lap("filtered sparse")

        def dev_row(i):
            lo = i * (i - 1) // 2
            return M[lo: lo + i].cpu().numpy().view(np.uint32)
        for i in (1, 49, 50, N // 2, N - 1):
            lo = i * (i - 1) // 2
            c, v = d.sparse_from_dense_device(M.data_ptr() + 4 * lo, lo, lo + i).row(i)
            row = dev_row(i)
            nz = np.nonzero(row)[0]
            assert np.array_equal(c, nz) and np.array_equal(v, row[nz])
        lap("sparse rows")
        row_cells = lambda i, cols: dev_row(i)[cols]                # noqa: E731
    # rows of the matrix straight from the definition (first rows, both sides of a clade boundary, the middle, the last clade, the last row)
    _definition_rows(S, g, k, f, N, cs, (1, 2, cs - 1, cs, cs + 1, N // 2, N - cs, N - 1), row_cells, device)
    lap("definition rows")
    lap.done()


def test_prefix_sharded_ranks_on_one_gpu(K, O, dev, tmp_path):
    """bench.py's multi-GPU scheme with the ranks run one after another on a single GPU:
    the partial matrices of the prefix-bucket shards add up to the unsharded matrix."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    N, cs, L, k = 200, 20, 20000, 18
    device = torch.device("cuda", dev)
    g = S.CladeGenomes(N, cs, L, seed=5, device=device)

    def run(rank, world):
        def km(i):
            x = S.kmers_of(g.sample(i), k)
            return x if world == 1 else x[((x >> 32) % world) == rank]
        arr = S.to_view_arrays(S.build_patterns(km, N, device))
        view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                           arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
        return K.DeviceDB(view, device=dev).all2all_dense()
    full = run(0, 1)
    for world in (2, 8):
        acc = np.zeros_like(full)
        for r in range(world):
            acc += run(r, world)
        assert np.array_equal(acc, full)


def _definition_rows(S, g, k, f, N, cs, rows, cell, device, ncols=1500):
    """Rows of the matrix straight from the definition, independent of patterns, trees and records: M[i][j] = |K_i ∩ K_j| over the samples'
    k-mer SETS.  `cell(i, cols)` returns the matrix's cells (i, cols) as a uint32 array.  The columns: the row's own clade and its
    neighbours, the first and the last clades, and a spread over the whole range (deriving all N k-mer sets again took half of the
    10 000 - 70 000-sample tests' time: VERDICT round 4, the GPU suite must fit the driver's limit)."""
    import torch
    rows = sorted(set(int(i) for i in rows if 0 < i < N))
    ks = {i: S.kmers_of(g.sample(i), k, f) for i in rows}
    spread = set(range(0, N, max(1, N // ncols)))
    colset = {i: set(c for c in (set(range(0, 2 * cs)) | set(range(max(0, i - 2 * cs), i)) | spread) if c < i) for i in rows}
    want = {i: {} for i in rows}
    for j in sorted(set().union(*colset.values())):
        kj = S.kmers_of(g.sample(j), k, f)
        for i in rows:
            if j in colset[i]:
                want[i][j] = int(torch.isin(kj, ks[i]).sum().item()) if kj.numel() and ks[i].numel() else 0
    for i in rows:
        cols = np.array(sorted(colset[i]), dtype=np.int64)
        assert np.array_equal(cell(i, cols), np.array([want[i][int(c)] for c in cols], dtype=np.uint32)), i


def _random_forest(rng, N, P, max_local, heavy_frac=0.2, zero_frac=0.2, chain_frac=0.0):
    """A random but valid pattern forest (not derived from genomes): pattern 0 is empty; every other
    pattern hangs under a random earlier pattern (or is a root) and owns 1..max_local ids larger than
    everything above it; with probability chain_frac the parent is the previous pattern (deep root paths that
    cross many blocks).  Returns pattern dict in the format of synth.build_patterns."""
    import torch
    parent = np.full(P, -1, dtype=np.int64)
    nsam = np.zeros(P, dtype=np.int64)
    last = np.full(P, -1, dtype=np.int64)
    locs = [np.zeros(0, dtype=np.int64)]
    w = np.zeros(P, dtype=np.int64)
    for p in range(1, P):
        for att in range(20):
            if att == 0 and p > 1 and rng.random() < chain_frac:
                par = p - 1
            else:
                par = int(rng.integers(0, p)) if rng.random() < 0.85 else 0
            lo = last[par] + 1 if par else 0
            if lo < N:
                break
        else:
            par, lo = 0, 0
        room = N - lo
        l = int(min(room, rng.integers(1, max_local + 1)))
        ids = np.sort(rng.choice(room, size=l, replace=False)) + lo
        parent[p] = par if par else -1
        nsam[p] = (nsam[par] if par else 0) + l
        last[p] = ids[-1]
        locs.append(ids.astype(np.int64))
        r = rng.random()
        w[p] = 0 if r < zero_frac else (int(rng.integers(2, 1 << int(rng.integers(8, 33)))) if r < zero_frac + heavy_frac else int(rng.integers(1, 4)))
    num_local = np.array([len(x) for x in locs], dtype=np.int64)
    lp = np.zeros(P + 1, dtype=np.int64)
    lp[1:] = np.cumsum(num_local)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    return {"num_kmers": t(w), "parent": t(parent), "num_samples": t(nsam), "num_local": t(num_local),
            "local_ptr": t(lp), "local_ids": t(np.concatenate(locs))}


@pytest.mark.parametrize("seed,N,P,max_local,chain", [(1, 2, 5, 1, 0), (2, 64, 300, 5, 0), (3, 65, 2000, 3, 0), (4, 700, 6000, 40, 0),
                                                      (5, 1024, 3000, 300, 0), (6, 2048, 4000, 64, 0), (7, 130, 20000, 2, 0),
                                                      (8, 1500, 500, 1200, 0), (9, 1000, 30000, 3, 0.9), (10, 1000, 60000, 2, 0.97),
                                                      (11, 4000, 20000, 3, 0.95), (12, 3000, 40000, 2, 0.995)])
def test_random_forests_bit_exact(K, O, dev, tmp_path, seed, N, P, max_local, chain):
    """Fuzz: arbitrary valid pattern forests (deep chains, long local lists, zero and huge weights, lists
    longer than 1024 ids -> v1 fallback) through every all2all path, against the oracle's tree form AND
    flat form."""
    import importlib
    S = importlib.import_module("kmerdb_amd.synth")
    rng = np.random.default_rng(seed)
    pat = _random_forest(rng, N, P, max_local, chain_frac=chain)
    arr = S.to_view_arrays(pat)
    path = str(tmp_path / "f.db")
    S.write_db(path, 18, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr)
    odb = O.OracleDB(path, skip_hashtables=True)
    exp = odb.all2all_dense()
    assert np.array_equal(odb.all2all_flat(), exp)
    view = K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    assert np.array_equal(d.all2all_dense(), exp)
    if chain and max_local <= 3:
        # root paths of hundreds to thousands of nodes stay on the block-record pipeline (chain table sized by the depth)
        assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp) and d.stats()["path"] == K.capi.PATH_RECORDS
    for fl in (K.capi.FLAG_FORCE_TILE, K.capi.FLAG_FORCE_GLOBAL_ATOMICS, K.capi.FLAG_FORCE_DIRECT):
        assert np.array_equal(d.all2all_dense(flags=fl), exp), fl
    acc = np.zeros_like(exp)
    for sh in range(3):
        acc += d.all2all_dense(shard=(sh, 3))
    assert np.array_equal(acc, exp)
    sp = d.all2all_sparse()
    for i in range(0, N, max(1, N // 7)):
        c, v = sp.row(i)
        row = O.tri_row(exp, i)
        nz = np.nonzero(row)[0]
        assert np.array_equal(c, nz) and np.array_equal(v, row[nz])


@pytest.mark.gpu
def test_bench_through_the_products_node_driver(dev):
    """`bench.py --driver node`: the line the driver's `--gpus N` run prints comes from the PRODUCT's multi-GPU path —
    kmdb_node_upload / kmdb_node_all2all_dense (csrc/node.hip) in one process — not from a Python re-implementation of it.  On the one-GPU box:
    (a) KMDB_NODE_FORCE_RCCL=1 --gpus 1: the RCCL half of the driver on a one-rank communicator (dlopen, ncclCommInitAll, the reduce-scatter of
    every step), the line's schema, figures per device from kmdb_node_device_stats; (b) --gpus 1 --shards 4: four prefix shards of ONE database
    one after the other on the device (the one-GPU anchor of a four-GPU run), checksum identity inside bench.py; (c) under a launcher with two
    ranks, rank 0 drives and rank 1 waits at the barriers (--gpus 1 there: the box has one device)."""
    import json
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--driver", "node", "--samples", "400", "--clade-size", "50", "--length", "20000", "--steps", "2", "--warmup", "1"]
    env = dict(os.environ, KMDB_NODE_FORCE_RCCL="1")
    r = subprocess.run(base + ["--gpus", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    last_json = lambda out: json.loads([ln for ln in out.strip().split("\n") if ln.startswith("{")][-1])      # noqa: E731  (RCCL's banner may follow the line)
    d = last_json(r.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["dtype"] == "u32" and d["config"]["driver"] == "node" and d["config"]["n_ranks_seen"] == 1
    assert d["config"]["rccl"] and d["config"]["per_rank"]["collective_ms"][0] > 0 and d["config"]["per_rank"]["call_ms"][0] > 0
    assert d["roofline"]["frac"] > 0 and d["value"] > 0
    r = subprocess.run(base + ["--gpus", "1", "--shards", "4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d4 = last_json(r.stdout)
    pr = d4["config"]["per_rank"]
    assert pr["shards"] == [4] and pr["block_records"][0] > 0 and pr["h2d_bytes"][0] > 0 and d4["config"]["rccl"] is None
    assert d4["config"]["patterns_rank0"] == d["config"]["patterns_rank0"]
    # two launcher ranks, one device: rank 0 is the node driver's process, rank 1 only keeps the launcher's rendezvous
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(29500 + os.getpid() % 1000)] + base[1:] + ["--gpus", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().split("\n") if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["config"]["driver"] == "node"


@pytest.mark.gpu
def test_more_than_65535_samples(K, O, dev, tmp_path):
    """Sample ids take 20 bits in the device layout (reference: 32-bit ids, src/types.h:15-18; its own 2019 collection data/pathogens.list
    has 40 715 samples).  (a) a random forest over 66 000 samples — local lists whose ids and deltas need 17 bits, long lists, deep
    chains — whole matrix against the oracle, block-record pipeline only (the HBM-atomics kernels keep 16-bit ids and refuse);
    (b) a clade collection of 70 000 samples: checksum identity, rows from the definition, new2all rows against the oracle."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    device = torch.device("cuda", dev)
    lap = _Laps("more_than_65535")
    # (a)
    N = 66000
    rng = np.random.default_rng(65536)
    pat = _random_forest(rng, N, 4000, 300, chain_frac=0.5)
    # local lists that JUMP over 65 536 ids at once: a gamma code of 33 - 39 bits, more than the decode kernel's 32-bit window holds (round 5
    # clamped such a code to 31 bits and read a wrong delta; the random forest above has no such list) — two ids, a short list with the jump in
    # the middle, one behind a run of consecutive ids, a long list (the second decode launch), and children that extend them
    import torch
    extra = [(-1, [3, 65990]), (-1, [10, 11, 65800, 65801]), (-1, list(range(100, 140)) + [65950]), (-1, list(range(200, 290)) + [65960, 65961]),
             (-1, [0, 65536]), (-1, [7, 65543, 65999])]
    P0 = int(pat["num_kmers"].numel())
    extra += [(P0 + 0, [65995]), (P0 + 1, [65900, 65999]), (P0 + 2, [65951])]
    par, nsam, nloc, ids, w = (pat[k].tolist() for k in ("parent", "num_samples", "num_local", "local_ids", "num_kmers"))
    for pp, lst in extra:
        par.append(pp); nloc.append(len(lst)); ids += lst; w.append(3)
        nsam.append(len(lst) + (nsam[pp] if pp >= 0 else 0))
    lp = np.zeros(len(par) + 1, dtype=np.int64)
    lp[1:] = np.cumsum(nloc)
    pat = {"num_kmers": torch.tensor(w), "parent": torch.tensor(par), "num_samples": torch.tensor(nsam), "num_local": torch.tensor(nloc),
           "local_ptr": torch.from_numpy(lp), "local_ids": torch.tensor(ids)}
    arr = S.to_view_arrays(pat)
    assert int(arr["last_sample_id"].max()) > 65535 and int(arr["num_samples"].max()) > 500 and int(arr["num_bits"].max()) > 4096
    path = str(tmp_path / "f.db")
    S.write_db(path, 18, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr)
    lap("forest")
    exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
    lap("oracle")
    view = K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    # (the 2.2 G cells are compared on the device: three copies of the 8.7 GB matrix through host memory and numpy were a minute of the test)
    E = torch.from_numpy(exp.view(np.int32)).to(device)
    lap("expected to device")
    M = torch.zeros(d.tri_size(), dtype=torch.int32, device=device)
    d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_NO_FALLBACK)
    st = d.stats()
    assert st["path"] == K.capi.PATH_RECORDS              # (no checksum identity here: the forest's heavy weights wrap the uint32 cells)
    assert torch.equal(M, E)
    M2 = torch.zeros_like(M)
    d.all2all_dense_device(M.data_ptr(), shard=(0, 2))
    d.all2all_dense_device(M2.data_ptr(), shard=(1, 2))
    M2 += M
    assert torch.equal(M2, E)
    del M2
    # the HBM-atomics kernel (32-bit ids on its global stack) takes such a collection too: it is the fallback of (c)
    d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_FORCE_GLOBAL_ATOMICS)
    assert d.stats()["path"] == K.capi.PATH_GLOBAL and torch.equal(M, E)
    lap("device matrix, two shards, HBM-atomics kernel")
    # the compaction of single rows on both sides of 65 536 (the host-matrix entry point — one more 8.7 GB array through host memory — has its
    # tests at 10 000 - 36 000 samples: the same device call and one copy)
    d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_NO_FALLBACK)
    for i in (1, 65535, 65536, N - 1):
        lo = i * (i - 1) // 2
        c, v = d.sparse_from_dense_device(M.data_ptr() + 4 * lo, lo, lo + i).row(i)
        row = O.tri_row(exp, i)
        nz = np.nonzero(row)[0]
        assert np.array_equal(c, nz) and np.array_equal(v, row[nz])
    d.close()
    del E, M, exp
    torch.cuda.empty_cache()
    # (c) a tree DEEPER than the block-record pipeline's chain table (4096 nodes on a root path) on more than 65 535 samples: round 5 had no
    # path for it at all (the fallback kept 16-bit ids: VERDICT round 5, missing 6); the reference has no such limit
    # (src/similarity_calculator.h:30-77).  A chain of 5000 and more nodes, one or two ids each, whole matrix against the oracle.
    rng = np.random.default_rng(5000)
    P = 5600
    parent = np.full(P, -1, dtype=np.int64)
    nsam = np.zeros(P, dtype=np.int64)
    last = np.full(P, -1, dtype=np.int64)
    locs = [np.zeros(0, dtype=np.int64)]
    tip, chain_done = 0, False
    for p in range(1, P):
        # one long chain (tip -> p adds one or two ids some steps further on, until the ids run out near N), and now and then — and from
        # there on — a leaf off an earlier node
        side = chain_done or (p > 3 and rng.random() < 0.05)
        for _ in range(100):
            par = int(rng.integers(1, p)) if side else tip
            lo = last[par] + 1 if par else 0
            l = int(rng.integers(1, 3))
            ids = lo + np.cumsum(rng.integers(1, 17, size=l)) - 1
            if ids[-1] < N:
                break
            side = chain_done = True
        assert ids[-1] < N
        if not side:
            tip = p
        parent[p] = par if par else -1
        nsam[p] = (nsam[par] if par else 0) + l
        last[p] = ids[-1]
        locs.append(ids.astype(np.int64))
    w = np.where(rng.random(P) < 0.3, 0, rng.integers(1, 5, size=P)).astype(np.int64)
    w[0] = 0
    num_local = np.array([len(x) for x in locs], dtype=np.int64)
    lp = np.zeros(P + 1, dtype=np.int64)
    lp[1:] = np.cumsum(num_local)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    pat = {"num_kmers": tt(w), "parent": tt(parent), "num_samples": tt(nsam), "num_local": tt(num_local), "local_ptr": tt(lp), "local_ids": tt(np.concatenate(locs))}
    arr = S.to_view_arrays(pat)
    par = arr["parent_id"]
    depth = np.zeros(par.size, np.int64)
    for p in range(1, par.size):
        depth[p] = depth[par[p]] + 1 if par[p] >= 0 else 1
    assert int(depth.max()) > 4200 and int(arr["num_samples"].max()) > 4200 and int(arr["last_sample_id"].max()) > 65535
    path = str(tmp_path / "deep.db")
    S.write_db(path, 18, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr)
    exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
    lap("deep forest + oracle")
    view = K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    E = torch.from_numpy(exp.view(np.int32)).to(device)
    M = torch.zeros(d.tri_size(), dtype=torch.int32, device=device)
    d.all2all_dense_device(M.data_ptr())
    assert d.stats()["path"] == K.capi.PATH_GLOBAL and "chain table" in d.fallback_reason()
    assert torch.equal(M, E)
    with pytest.raises(K.KmdbError, match="chain table"):
        d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_NO_FALLBACK)
    lap("deep forest on the device")
    d.close()
    del exp, M, E
    lap("sparse rows")
    # (b)
    N, cs, L, k = 70000, 50, 200, 18
    g, pat = S.synth_database(N, cs, L, k=k, seed=17, device=device)
    arr = S.to_view_arrays(pat)
    lap("clade database")
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    lap("hashtables")
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"], bucket_offset=tables[0], slots=tables[1])
    d = K.DeviceDB(view, device=dev, with_hashtables=True)
    M = torch.zeros(d.tri_size(), dtype=torch.int32, device=device)
    d.all2all_dense_device(M.data_ptr(), flags=K.capi.FLAG_NO_FALLBACK)
    st = d.stats()
    assert st["path"] == K.capi.PATH_RECORDS and st["n_records"] > 0
    total = sum(int(M[o: o + (1 << 28)].to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item()) for o in range(0, M.numel(), 1 << 28))
    assert total == st["sum_pairs"]
    def cells(i, cols):
        o = i * (i - 1) // 2
        return M[o: o + i][torch.from_numpy(cols).to(device)].cpu().numpy().view(np.uint32)
    lap("upload, call, checksum")
    _definition_rows(S, g, k, 1.0, N, cs, (1, cs, 65535, 65536, 65537, N - cs, N - 1), cells, device)
    del M
    lap("definition rows")
    # (new2all rows are checked on a subset of the samples: the first and last clades, both sides of 65 536, a spread over all of them)
    sub = sorted(set(range(0, 2 * cs)) | set(range(65536 - 2 * cs, 65536 + 2 * cs)) | set(range(N - 2 * cs, N)) | set(range(0, N, 100)))
    allk = torch.cat([S.kmers_of(g.sample(j), k) for j in sub])
    sid = torch.repeat_interleave(torch.tensor(sub, device=device), torch.tensor([pat["sample_counts"][j] for j in sub], device=device))
    sub = np.array(sub)
    # new2all: members on both sides of 65 536, fresh strains of the last clades, an unrelated genome, an empty query
    g_more = S.CladeGenomes(N + 100, cs, L, seed=17, device=device)
    other = S.CladeGenomes(10, 5, L, seed=77, device=device)
    qs = [S.kmers_of(g.sample(i), k).cpu().numpy().view(np.uint64) for i in (0, 65535, 65536, N - 1)]
    qs += [S.kmers_of(g_more.sample(i), k).cpu().numpy().view(np.uint64) for i in (N, N + 99)]
    qs += [S.kmers_of(other.sample(2), k).cpu().numpy().view(np.uint64), np.zeros(0, np.uint64)]
    got = d.new2all(qs)
    for qi, q in enumerate(qs):
        hit = torch.isin(allk, torch.from_numpy(q.view(np.int64)).to(device))
        want = torch.bincount(sid[hit], minlength=N).cpu().numpy().astype(np.uint32)
        assert np.array_equal(got[qi][sub], want[sub]), qi
    assert got[1, 65535] == qs[1].size and got[2, 65536] == qs[2].size and got[3, N - 1] == qs[3].size
    sp = d.new2all_sparse(qs)
    for qi in range(len(qs)):
        c, v = sp.row(qi)
        nz = np.nonzero(got[qi])[0]
        assert np.array_equal(c, nz) and np.array_equal(v, got[qi][nz])
    d.close()
    lap("new2all")
    lap.done()


@pytest.mark.parametrize("rowmode", ["0", "1"])
def test_pools_too_small_are_enlarged_and_the_call_repeated(K, O, dev, tmp_path, rowmode):
    """The record pools are sized from a 1-in-1024 sample; a pool that turns out too small is enlarged and the call repeated
    (no test forced that path).  Pools of 1 % of the estimate, few streams and many (the per-block-row chunks):
    the first call overflows every pool several times over and still returns the oracle's matrix; so does the sliced call."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    N, cs, L, k = 1200, 50, 4000, 18
    device = torch.device("cuda", dev)
    g, pat = S.synth_database(N, cs, L, k=k, seed=5, device=device)
    arr = S.to_view_arrays(pat)
    path = str(tmp_path / "s.db")
    S.write_db_fast(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr, device=device)
    exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"])
    env = {"KMDB_POOL_PERCENT": "1", "KMDB_ROW_MODE": rowmode, "KMDB_BLOCK_WIDTH": "32"}
    try:
        os.environ.update(env)
        d = K.DeviceDB(view, device=dev)
        got = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
        assert np.array_equal(got, exp) and d.stats()["path"] == K.capi.PATH_RECORDS
        assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp) and d.stats()["sized_call"] == 0
        d.close()
        os.environ["KMDB_SLICES"] = "5"                      # the call takes the pattern stream in five passes
        d = K.DeviceDB(view, device=dev)
        assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp) and d.stats()["path"] == K.capi.PATH_RECORDS
        assert d.stats()["n_records"] > 0
        d.close()
    finally:
        for name in list(env) + ["KMDB_SLICES"]:
            os.environ.pop(name, None)


def test_patterns_that_touch_every_block_of_many(K, O, dev):
    """One conserved k-mer shared by most samples is a pattern whose full list touches EVERY block: at more than 32 768 samples
    that is more than 512 (block, mask) entries — the limit at which round 2's wide-node kernel gave the whole database up (ADVICE
    round 2).  Lists are now as long as there are blocks: a forest of such patterns (a root with one id in every block and a chain of
    children that fill the blocks in) stays on the block-record pipeline and equals the flat-form definition computed here on the
    host (reference similarity_calculator.cpp:596-638: every pattern adds its weight to all pairs of its full list)."""
    import torch
    N, step = 36000, 40
    ids0 = np.arange(0, N, step, dtype=np.int64)                 # 900 ids: one in every block of any width >= 40, two in most
    locs = [np.zeros(0, dtype=np.int64), ids0]
    parent, w = [-1, -1], [0, 3]
    # children: ids above the root's last id cannot exist (ids ascend along a path), so the chain grows at the top end only; siblings
    # of the root pattern cover other residues
    for r in (1, 7, 13):
        locs.append(np.arange(r, N, step, dtype=np.int64)); parent.append(-1); w.append(1 + r)
    top = int(ids0[-1])
    chain_par = 1
    for j in range(1, 30):
        if top + j >= N:
            break
        locs.append(np.array([top + j], dtype=np.int64)); parent.append(chain_par); w.append(j % 3); chain_par = len(locs) - 1
    P = len(locs)
    nloc = np.array([len(x) for x in locs], dtype=np.int64)
    nsam = np.zeros(P, dtype=np.int64)
    for p in range(1, P):
        nsam[p] = nloc[p] + (nsam[parent[p]] if parent[p] >= 0 else 0)
    lp = np.zeros(P + 1, dtype=np.int64); lp[1:] = np.cumsum(nloc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64)))      # noqa: E731
    pat = {"num_kmers": t(w), "parent": t(parent), "num_samples": t(nsam), "num_local": t(nloc), "local_ptr": t(lp), "local_ids": t(np.concatenate(locs))}
    import importlib
    S = importlib.import_module("kmerdb_amd.synth")
    arr = S.to_view_arrays(pat)
    view = K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                       arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    got = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
    st = d.stats()
    assert st["path"] == K.capi.PATH_RECORDS and st["n_wide"] >= 4
    # flat form on the host: full lists by walking the parents
    exp = np.zeros(N * (N - 1) // 2, dtype=np.uint32)
    for p in range(1, P):
        if w[p] == 0:
            continue
        full, q = [], p
        while q >= 0:
            full.append(locs[q]); q = parent[q]
        full = np.sort(np.concatenate(full))
        for a in range(1, full.size):
            i = int(full[a])
            exp[i * (i - 1) // 2 + full[:a]] += np.uint32(w[p])
    assert np.array_equal(got, exp)
    assert st["sum_pairs"] == int(exp.astype(np.uint64).sum())
    d.close()


@pytest.mark.parametrize("form", ["packed", "unpacked"])
def test_few_streams_record_forms(K, O, dev, tmp_path, form):
    """The few-streams path (at most 2048 block pairs: BASELINE configs[1]) moves its block records in one of two forms: packed (block
    width <= 54: 16 bytes, the weight digit in the column word's spare bits, the key words stay behind in the one-pass sort, apply step by
    stream jobs) and unpacked (KMDB_REC_PACKED=0, or any width above 54: 16 + 4 bytes, stream jobs).  Random forests with weights of up to 32 bits (one to four digits of 8 - 16 bits) at widths 32 / 50 / 54 /
    64 against the oracle: whole call, warm call, slices of the pattern stream (reference src/similarity_calculator.cpp:42-438)."""
    import importlib
    S = importlib.import_module("kmerdb_amd.synth")
    env = {"packed": {}, "unpacked": {"KMDB_REC_PACKED": "0"}}[form]
    keys = ("KMDB_REC_PACKED", "KMDB_BLOCK_WIDTH", "KMDB_ROW_MODE")
    saved = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        for seed, N, P, max_local, chain in ((31, 1000, 6000, 60, 0.2), (32, 2048, 3000, 300, 0.5), (33, 640, 20000, 8, 0.0)):
            rng = np.random.default_rng(seed)
            pat = _random_forest(rng, N, P, max_local, heavy_frac=0.4, chain_frac=chain)
            arr = S.to_view_arrays(pat)
            path = str(tmp_path / ("r%d.db" % seed))
            S.write_db(path, 18, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr)
            exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
            view = K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                               arr["data_offset"], arr["data"])
            for width in ("32", "50", "54", "64"):
                os.environ["KMDB_BLOCK_WIDTH"] = width
                d = K.DeviceDB(view, device=dev)
                got = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
                st = d.stats()
                assert st["path"] == K.capi.PATH_RECORDS and st["width"] == int(width), (seed, width, st)
                assert np.array_equal(got, exp), (form, seed, width)
                assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp) and d.stats()["sized_call"] == 0, (form, seed, width)
                acc = np.zeros_like(exp)
                for sh in range(2):
                    acc += d.all2all_dense(shard=(sh, 2), flags=K.capi.FLAG_NO_FALLBACK)
                assert np.array_equal(acc, exp), (form, seed, width)
                d.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("l2min", ["11", "24"])
def test_second_level_above_the_block_records(K, O, dev, tmp_path, l2min):
    """The nodes with many blocks (KMDB_L2_MIN, default 24) write (node, block, mask) entries instead of their c (c + 1) / 2 block
    records and are joined per tile (l2_* kernels, reference src/similarity_calculator.cpp:42-438 at N = 10 000).  Forced here on small
    inputs (row mode, width 32): random forests against the oracle — whole call, warm call, slices of the pattern stream — the arrays of
    the second level far too small (doubled and the call repeated), a pattern in every block (definition on the host), a clade
    collection in prefix shards, and the same with the second level switched off."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    device = torch.device("cuda", dev)
    env = {"KMDB_ROW_MODE": "1", "KMDB_L2_MIN": l2min, "KMDB_BLOCK_WIDTH": "32"}
    try:
        os.environ.update(env)
        for seed, N, P, max_local, chain, tiny in ((21, 2048, 4000, 64, 0.0, False), (22, 1500, 500, 1200, 0.0, False), (23, 3000, 20000, 40, 0.6, True),
                                                   (24, 8000, 3000, 300, 0.3, False)):
            rng = np.random.default_rng(seed)
            pat = _random_forest(rng, N, P, max_local, chain_frac=chain)
            arr = S.to_view_arrays(pat)
            path = str(tmp_path / ("f%d.db" % seed))
            S.write_db(path, 18, 1.0, ["s%d" % i for i in range(N)], [1] * N, arr)
            exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
            view = K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                               arr["data_offset"], arr["data"])
            if tiny:
                os.environ["KMDB_POOL_PERCENT"] = "1"
            d = K.DeviceDB(view, device=dev)
            got = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
            st = d.stats()
            assert st["path"] == K.capi.PATH_RECORDS and st["n_joined"] > 0, (seed, st)
            assert np.array_equal(got, exp), seed
            assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp) and d.stats()["sized_call"] == 0
            acc = np.zeros_like(exp)
            for sh in range(3):
                acc += d.all2all_dense(shard=(sh, 3), flags=K.capi.FLAG_NO_FALLBACK)
            assert np.array_equal(acc, exp), seed
            joined = st["n_joined"]
            d.close()
            os.environ.pop("KMDB_POOL_PERCENT", None)
            os.environ["KMDB_L2"] = "0"
            d = K.DeviceDB(view, device=dev)
            assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp) and d.stats()["n_joined"] == 0
            assert d.stats()["n_records"] > st["n_records"] or joined == 0
            d.close()
            os.environ.pop("KMDB_L2", None)
        # a pattern in every block: 250 blocks of width 32, lists of 200 - 250 entries; flat form on the host
        N, step = 8000, 40
        ids0 = np.arange(0, N, step, dtype=np.int64)
        locs, parent, w = [np.zeros(0, dtype=np.int64), ids0], [-1, -1], [0, 3]
        for r in (1, 7, 13):
            locs.append(np.arange(r, N, step, dtype=np.int64)); parent.append(-1); w.append(200 + r)          # (weights of two base-128 digits)
        top, chain_par = int(ids0[-1]), 1
        for j in range(1, 30):
            if top + j >= N:
                break
            locs.append(np.array([top + j], dtype=np.int64)); parent.append(chain_par); w.append(j % 3); chain_par = len(locs) - 1
        P = len(locs)
        nloc = np.array([len(x) for x in locs], dtype=np.int64)
        nsam = np.zeros(P, dtype=np.int64)
        for q in range(1, P):
            nsam[q] = nloc[q] + (nsam[parent[q]] if parent[q] >= 0 else 0)
        lp = np.zeros(P + 1, dtype=np.int64); lp[1:] = np.cumsum(nloc)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64)))      # noqa: E731
        pat = {"num_kmers": t(w), "parent": t(parent), "num_samples": t(nsam), "num_local": t(nloc), "local_ptr": t(lp), "local_ids": t(np.concatenate(locs))}
        arr = S.to_view_arrays(pat)
        view = K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                           arr["data_offset"], arr["data"])
        d = K.DeviceDB(view, device=dev)
        got = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
        assert d.stats()["n_joined"] >= 4
        exp = np.zeros(N * (N - 1) // 2, dtype=np.uint32)
        for q in range(1, P):
            if w[q] == 0:
                continue
            full, y = [], q
            while y >= 0:
                full.append(locs[y]); y = parent[y]
            full = np.sort(np.concatenate(full))
            for a in range(1, full.size):
                i = int(full[a])
                exp[i * (i - 1) // 2 + full[:a]] += np.uint32(w[q])
        assert np.array_equal(got, exp)
        d.close()
        # a clade collection, whole and in prefix-bucket shards (the pruned trees of kmdb_db_upload_shard)
        N, cs, L, k = 1600, 50, 3000, 18
        g, pat = S.synth_database(N, cs, L, k=k, seed=31, device=device)
        arr = S.to_view_arrays(pat)
        path = str(tmp_path / "c.db")
        S.write_db_fast(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr, device=device)
        exp = O.OracleDB(path, skip_hashtables=True).all2all_dense()
        tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
        view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                           arr["data_offset"], arr["data"], bucket_offset=tables[0], slots=tables[1])
        d = K.DeviceDB(view, device=dev)
        assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), exp)
        whole = d.stats()["n_joined"]
        assert whole > 0 or l2min == "24"
        d.close()
        acc = np.zeros_like(exp)
        for s_ in range(3):
            d = K.DeviceDB(view, device=dev, prefix_shard=(s_, 3))
            acc += d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
            d.close()
        assert np.array_equal(acc, exp)
    finally:
        for name in list(env) + ["KMDB_POOL_PERCENT", "KMDB_L2"]:
            os.environ.pop(name, None)


def test_degenerate_databases(K, O, dev, tmp_path):
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    z = lambda n: torch.zeros(n, dtype=torch.int64)     # noqa: E731
    # only the empty pattern, one sample
    pat = {"num_kmers": z(1), "parent": torch.tensor([-1]), "num_samples": z(1), "num_local": z(1),
           "local_ptr": z(2), "local_ids": z(0)}
    arr = S.to_view_arrays(pat)
    view = K.make_view(18, 1, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    assert d.all2all_dense().size == 0 and d.all2all_sparse().nnz == 0
    # three samples, singleton patterns only: no pair is shared
    pat = {"num_kmers": torch.tensor([0, 5, 7, 9]), "parent": torch.tensor([-1, -1, -1, -1]),
           "num_samples": torch.tensor([0, 1, 1, 1]), "num_local": torch.tensor([0, 1, 1, 1]),
           "local_ptr": torch.tensor([0, 0, 1, 2, 3]), "local_ids": torch.tensor([0, 1, 2])}
    arr = S.to_view_arrays(pat)
    view = K.make_view(18, 3, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    assert np.array_equal(d.all2all_dense(), np.zeros(3, np.uint32))
    # a bad view is refused, not crashed on
    bad = arr["parent_id"].copy()
    bad[1] = 3
    view = K.make_view(18, 3, arr["num_kmers"], bad, arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    with pytest.raises(K.KmdbError, match="parent_id"):
        K.DeviceDB(view, device=dev)


def test_bench_contract_single_and_two_ranks(dev, tmp_path):
    """bench.py prints ONE JSON line with the contract's keys (--full: with the CPU baseline) and --dump-outputs writes the matrix of
    the last timed call; the multi-rank path (prefix-bucket shards + matrix reduce) runs end to end with two ranks sharing this GPU over
    gloo and reproduces the single-rank checksum structure (the bench asserts sum(M) == sum_p w_p C(n_p,2) over all ranks)."""
    import json
    import sys
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--length", "60000", "--cpu-sample-length", "20000",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["dtype"] == "u32" and "workload" in d["config"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"])
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(d["cpu_baseline"])
    # wall-clock half of the metric: upload, first call, both together; and the fast path ran
    assert set(("upload_s", "cold_call_ms", "cold_total_s", "warm_ms")) <= set(d["wall"])
    assert d["config"]["path"] == "block-record pipeline" and d["roofline"]["block_records_per_launch"] > 0
    if d["cpu_baseline"]["kind"] == "reference":
        assert "full" in d["cpu_baseline"]["sample"]           # the reference timed on the whole database of the timed workload
    m = np.load(str(tmp_path / "out" / "matrix.npy"))
    n = d["config"]["samples"]
    assert m.dtype == np.float64 and m.shape == (n * (n - 1) // 2,)
    assert abs(m.sum() - d["value"] * d["ms_per_step"] * 1e-3) <= 1e-9 * m.sum()      # value = sum of the matrix per second of one step
    # `--gpus 2` with NO launcher: bench.py starts its own two ranks (weak scaling: per-rank databases)
    # (strong scaling with the reduce to rank 0 ran here too until round 5: its two halves are the runs below; the suite has a time limit)
    for scaling, collective in (("weak", "reduce"), ("strong", "reduce_scatter")):
        r2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "c2", "--scaling", scaling,
                             "--collective", collective, "--length", "30000" if scaling == "weak" else "60000", "--steps", "2", "--warmup", "1"],
                            capture_output=True, text=True, env=env, timeout=900)
        assert r2.returncode == 0, r2.stderr[-3000:]
        lines = [ln for ln in r2.stdout.splitlines() if ln.strip().startswith("{")]
        assert len(lines) == 1
        d2 = json.loads(lines[0])
        assert d2["n_gpus"] == 2 and d2["scaling"] == scaling and d2["config"]["genome_length_bp"] == 60000
        assert d2["config"]["path"] == "block-record pipeline"
        # all runs cover a 60 kbp genome set of the same model: two prefix shards do the same total work
        assert abs(d2["value"] * d2["ms_per_step"] - d["value"] * d["ms_per_step"]) / (d["value"] * d["ms_per_step"]) < 1e-9
        pr = d2["config"]["per_rank"]
        assert d2["config"]["n_ranks_seen"] == 2 and len(pr["call_ms"]) == 2 and len(pr["collective_ms"]) == 2 and min(pr["call_ms"]) > 0
    # with more than one GPU and no --workload the job is BASELINE configs[2]'s: 10 000 samples, weak scaling (here at a toy genome length)
    r3 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--length", "2000", "--steps", "1", "--warmup", "1"],
                        capture_output=True, text=True, env=env, timeout=900)
    assert r3.returncode == 0, r3.stderr[-3000:]
    d3 = json.loads([ln for ln in r3.stdout.splitlines() if ln.strip().startswith("{")][0])
    assert d3["n_gpus"] == 2 and d3["scaling"] == "weak" and d3["config"]["samples"] == 10000 and d3["config"]["workload"].startswith("c3gpu: 10000 synthetic")
    assert d3["config"]["genome_length_bp"] == 4000 and d3["config"]["n_ranks_seen"] == 2


@pytest.mark.parametrize("extra", [["--collective", "reduce"], ["--collective", "reduce_scatter"], ["--mode", "all2all-sp", "--samples", "600"]])
def test_bench_rccl_branch_on_a_one_rank_group(dev, extra):
    """The `--backend nccl` branch of bench.py (what the driver's --gpus N run executes) on a one-GPU box: `--one-rank-group` builds a
    ONE-rank RCCL process group and runs the multi-rank code as it is — init_process_group(nccl, device_id), the int32 reduce /
    reduce_scatter_tensor of every step on the call's stream with events around it, the float64 all_reduce / all_gather of the figures,
    barrier, destroy — and the line's checksum identity holds over the collective's output."""
    import json
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--one-rank-group", "--length", "20000", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-extra"] + extra, capture_output=True, text=True, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][0])
    assert d["n_gpus"] == 1 and d["config"]["rccl"] not in (None, "unknown") and d["value"] > 0
    if "--mode" not in extra:
        pr = d["config"]["per_rank"]
        assert d["config"]["n_ranks_seen"] == 1 and pr["backend"] == "nccl" and pr["call_ms"][0] > 0 and pr["collective_ms"][0] > 0


def test_bench_one_gpu_share_of_configs2(dev):
    """BASELINE configs[2] (10 000 genomes of 5 Mbp over 8 GPUs) at its real per-GPU size: `--workload c3gpu` = 10 000 samples x 625 kbp,
    140 M patterns, more than 2^31 local ids in the tree, 1.08 G block records — ONE pass of the block-record pipeline (record pools
    beyond 2^31 slots on the many-streams path).  bench.py itself asserts the checksum identity over the whole 50 M-cell matrix
    (sum M == sum_p w_p C(n_p, 2)) and warm == cold."""
    import json
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c3gpu", "--no-cpu-baseline", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, env=dict(os.environ, KMDB_VERBOSE="1"), timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][0])
    assert d["config"]["samples"] == 10000 and d["config"]["genome_length_bp"] == 625000 and d["config"]["path"] == "block-record pipeline"
    # (round 4: 1.08 G block records; since round 5 the nodes with 24 blocks or more are joined per tile instead — 0.62 G records written)
    assert d["roofline"]["block_records_per_launch"] > 5 * 10 ** 8 and d["roofline"]["nodes_joined_per_tile"] > 10 ** 5
    assert "slices of the pattern stream" not in r.stderr, "one GPU's share of configs[2] should be one pass"


@pytest.mark.parametrize("mode", ["all2all-sp", "new2all", "db2db"])
def test_bench_secondary_modes(dev, mode):
    """`bench.py --mode`: the all2all-sp / new2all / db2db rows as driver-runnable lines in the same contract; each run checks a
    whole-output identity and (oracle/_ref present) compares every row with the real reference's output."""
    import json
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--mode", mode, "--samples", "600", "--length", "20000", "--queries", "24",
                        "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "wall"):
        assert k in d, k
    assert d["config"]["mode"] == mode and d["value"] > 0 and d["roofline"]["algorithmic_bytes_per_launch"] > 0
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"])
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "ref_driver")):
        assert d["cpu_baseline"]["kind"] == "reference" and "compared equal" in d["cpu_baseline"]["sample"]


def test_bench_all2all_sp_two_ranks(dev):
    """BASELINE configs[3] shape: `bench.py --mode all2all-sp --gpus 2` (two self-started ranks sharing this GPU over gloo): per-rank
    prefix-bucket shards, reduce of the partial matrices, per-rank compaction of its chunk of the triangle.  Same non-zeros and the same
    k-mer pair comparisons as the one-rank line on the same genomes (which compares every row with the real reference)."""
    import json
    import sys
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "all2all-sp", "--samples", "600", "--steps", "2", "--warmup", "1"]
    r1 = subprocess.run(base + ["--length", "20000"], capture_output=True, text=True, env=env, timeout=900)
    assert r1.returncode == 0, r1.stderr[-3000:]
    d1 = json.loads([ln for ln in r1.stdout.splitlines() if ln.strip().startswith("{")][0])
    r2 = subprocess.run(base + ["--length", "10000", "--gpus", "2", "--backend", "gloo"], capture_output=True, text=True, env=env, timeout=900)
    assert r2.returncode == 0, r2.stderr[-3000:]
    lines = [ln for ln in r2.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1
    d2 = json.loads(lines[0])
    assert d2["n_gpus"] == 2 and d2["config"]["mode"] == "all2all-sp" and d2["config"]["genome_length_bp"] == 20000
    assert d2["config"]["nnz"] == d1["config"]["nnz"]
    assert abs(d2["value"] * d2["ms_per_step"] - d1["value"] * d1["ms_per_step"]) / (d1["value"] * d1["ms_per_step"]) < 1e-9


def test_new2all_synthetic_scale(K, O, dev, tmp_path):
    """new2all on a bench-shaped database (1000 samples) with synthetic hashtables: members, fresh strains of
    known clades, an unrelated genome and an empty query, dense and sparse, against the oracle and the
    real reference."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    N, cs, L, k = 1000, 50, 12000, 18
    device = torch.device("cuda", dev)
    g, pat = S.synth_database(N, cs, L, k=k, seed=31, device=device)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    path = str(tmp_path / "s.db")
    S.write_db(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr,
               kmers_count=int(pat["dictionary"].numel()), tables=tables)
    g_more = S.CladeGenomes(N + 100, cs, L, seed=31, device=device)          # strains 1000.. are new members of clades 20, 21
    other = S.CladeGenomes(10, 5, L, seed=77, device=device)
    qs = [S.kmers_of(g.sample(i), k).cpu().numpy().view(np.uint64) for i in (0, 499, 999)]
    qs += [S.kmers_of(g_more.sample(i), k).cpu().numpy().view(np.uint64) for i in (1000, 1049)]
    qs += [S.kmers_of(other.sample(2), k).cpu().numpy().view(np.uint64), np.zeros(0, np.uint64)]
    o = O.OracleDB(path)
    exp = np.stack([o.one2all(q) for q in qs])
    d = K.DeviceDB(K.HostDB(path), device=dev, with_hashtables=True)
    got = d.new2all(qs)
    assert np.array_equal(got, exp)
    assert got[0, 0] == qs[0].size and got[2, 999] == qs[2].size
    sp = d.new2all_sparse(qs)
    for i in range(len(qs)):
        c, v = sp.row(i)
        nz = np.nonzero(exp[i])[0]
        assert np.array_equal(c, nz) and np.array_equal(v, exp[i][nz])
    if O.have_ref():
        O.write_kmers_bin(str(tmp_path / "q.bin"), k, 1.0, [("q%d" % i, q) for i, q in enumerate(qs)])
        rows, _ = O.ref_one2all(path, str(tmp_path / "q.bin"), str(tmp_path / "o.u32"), 4)
        assert np.array_equal(rows.reshape(len(qs), N), exp)
    # all2all of the same upload still works (hashtables do not disturb it)
    assert np.array_equal(d.all2all_dense(), o.all2all_dense())


@pytest.mark.gpu
def test_new2all_thousand_queries_vs_ten_thousand_samples(K, O, dev, tmp_path, monkeypatch):
    """BASELINE.json configs[4] in shape: 1000 queries (fresh strains of known clades) against a 10 000-sample k=18 database,
    streamed in batches; genome length scaled down so that the oracle checks every row.  Also the sequence-text entry point
    with a batch far over its per-piece base budget (the engine cuts it, rows are independent)."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    N, cs, L, k, NQ = 10000, 50, 600, 18, 1000
    device = torch.device("cuda", dev)
    g, pat = S.synth_database(N, cs, L, k=k, seed=41, device=device)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"], bucket_offset=tables[0], slots=tables[1])
    d = K.DeviceDB(view, device=dev, with_hashtables=True)
    g_more = S.CladeGenomes(N + NQ, cs, L, seed=41, device=device)          # strains N.. are new members of clades 200..219
    codes = [g_more.sample(N + i) for i in range(NQ)]
    qs = [S.kmers_of(c, k).cpu().numpy().view(np.uint64) for c in codes]
    got = np.concatenate([d.new2all(qs[b: b + 256]) for b in range(0, NQ, 256)])
    path = str(tmp_path / "s.db")
    S.write_db(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)
    o = O.OracleDB(path)
    exp = np.stack([o.one2all(q) for q in qs])
    assert np.array_equal(got, exp) and int(exp.sum()) > 0
    # sequence text, 1000 queries of 600 bases with a 5000-base budget per piece
    monkeypatch.setenv("KMDB_N2A_BASES_PER_PIECE", "5000")
    texts = ["".join("ACGT"[int(x)] for x in c.cpu().numpy()) for c in codes]
    rows, cnt = d.new2all_seq(texts)
    assert np.array_equal(rows, exp) and np.array_equal(cnt, np.array([q.size for q in qs], dtype=np.uint64))


@pytest.mark.gpu
def test_integration_glue_inside_the_reference(golden_dir, tmp_path):
    """integration/kmdb_bridge.h compiled against the unmodified reference headers and translation units
    (oracle/Makefile -> oracle/_ref/bridge_driver): the database is loaded by the reference's own deserialize, flattened by
    the bridge, run by libkmdb_amd.so, and the outputs equal the reference's golden outputs / its own one2all."""
    exe = os.path.join(ROOT, "oracle", "_ref", "bridge_driver")
    from conftest import require_ref_or_skip
    require_ref_or_skip(exe, "oracle/_ref/bridge_driver is built only where /root/reference exists")
    for stem in ("virus_k18", "clade64_k25_f01"):
        out = str(tmp_path / (stem + ".u32"))
        r = subprocess.run([exe, "all2all", os.path.join(golden_dir, stem + ".db"), out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert np.array_equal(np.fromfile(out, dtype=np.uint32), _ref_dense(golden_dir, stem))
    out = str(tmp_path / "sp.txt")
    r = subprocess.run([exe, "all2all_sp", os.path.join(golden_dir, "clade64.db"), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, "rb").read() == open(os.path.join(golden_dir, "clade64.a2a_sp.ref.txt"), "rb").read()
    r = subprocess.run([exe, "new2all", os.path.join(golden_dir, "clade64.db"), str(tmp_path / "row.u32")], capture_output=True, text=True)
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr[-2000:]
    # the -min / -max options parsed by the reference's own Params, translated by the bridge, applied on the device; the driver
    # compares the rows with the reference's CombinedFilter on the unfiltered rows, and the synth case equals the reference's golden
    for stem, opts in (("clade64", ["-min", "jaccard:0.02", "-max", "mash:0.2"]), ("virus_k18", ["-min", "ani-shorter:0.9", "-min", "num-kmers:100"]),
                       ("clade64_k25_f01", ["-max", "cosine:0.5", "-min", "min:0.01"]), ("synth_k21", ["-max", "39", "-min", "num-kmers:31"])):
        out = str(tmp_path / (stem + ".flt.txt"))
        r = subprocess.run([exe, "all2all_sp_filtered", os.path.join(golden_dir, stem + ".db"), out] + opts, capture_output=True, text=True)
        assert r.returncode == 0 and "identical to the reference's CombinedFilter" in r.stdout, r.stdout + r.stderr[-2000:]
    want = [ln.split(b",", 2)[2] for ln in open(os.path.join(golden_dir, "synth.a2a.sparse.above-below"), "rb").read().split(b"\n")[2:] if ln]
    assert open(out, "rb").read().split(b"\n")[:len(want)] == want


@pytest.mark.gpu
def test_randomised_stress_of_the_block_record_pipeline(dev):
    """profiles/r02_fuzz_stress.py: random forests x random block widths (odd ones too, which the width search never
    picks) x both front halves, against the v1 kernels that the tests above pin to the oracle."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "r02_fuzz_stress.py"), "60", "2026"], capture_output=True,
                       text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "60 cases, 0 mismatches" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("stem,k,fraction", [("virus_k18", 18, 1.0), ("synth_k21", 21, 1.0), ("virus_k24", 24, 1.0),
                                              ("virus_k25_f01_part1", 25, 0.1), ("virus_k18_f01", 18, 0.1)])
def test_device_side_extraction_fuzz(K, golden_dir, dev, stem, k, fraction):
    """random sequences (both cases, U, invalid symbols, record breaks, homopolymers) through kmdb_new2all_batch_seq and
    through the host loader + kmdb_new2all_batch: same unique k-mer counts, same similarity rows, for several k and with
    the minhash filter."""
    path = os.path.join(golden_dir, stem + ".db")
    d = K.DeviceDB(K.HostDB(path), device=dev, with_hashtables=True)
    rng = np.random.default_rng(k * 1000 + int(fraction * 10))
    genome = open(os.path.join(golden_dir, "test/virus/data/MT159713.fasta")).read().split("\n", 1)[1].replace("\n", "")
    alphabet = np.frombuffer(b"ACGTacgtUuNn-\n", dtype=np.uint8)
    texts = []
    for q in range(24):
        n = int(rng.integers(0, 4000))
        if q % 3 == 0:                                   # pieces of a real genome (hits in the virus databases) with noise
            a = int(rng.integers(0, len(genome) - n - 1))
            b = bytearray(genome[a:a + n].encode())
            for pos in rng.integers(0, max(1, n), size=n // 200):
                if n:
                    b[int(pos)] = int(alphabet[int(rng.integers(0, len(alphabet)))])
            texts.append(bytes(b))
        elif q % 3 == 1:
            p = np.array([8, 8, 8, 8, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1], dtype=float)
            texts.append(alphabet[rng.choice(len(alphabet), size=n, p=p / p.sum())].tobytes())
        else:
            texts.append((b"A" * int(rng.integers(0, 3 * k))) + b"\n" + (b"ACGT" * int(rng.integers(0, 40))))
    host = []
    for t in texts:
        parts = [K.extract_kmers(rec, k, fraction) for rec in t.split(b"\n")] if t else []
        host.append(K.sort_unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64))
    got, cnt = d.new2all_seq(texts, fraction=fraction)
    assert [int(c) for c in cnt] == [h.size for h in host]
    assert np.array_equal(got, d.new2all(host))
    assert got.any() or not stem.startswith("virus")          # the genome pieces hit the virus databases
