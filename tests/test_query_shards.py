"""Query shards: new2all / one2all over the GPUs of a node (kmdb_db_upload_query_shard, kmdb_new2all_batch*_device, kmdb_node_new2all_*,
`new2all -gpus N`, `one2all -gpus N`).  The host plan and the split of k-mer queries run without a GPU; everything else is marked gpu.
All comparisons are exact: every k-mer belongs to one prefix bucket (bucket = kmer >> 32, reference src/types.h:25-27), so the uint32 rows of
the shards sum to the rows of the whole database."""
import ctypes
import lzma
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported(K):
    """the additive part of the ABI: every new function of include/kmdb_amd.h is in capi.EXPORTS and in the library, the version stays 8"""
    new = ["kmdb_db_upload_query_shard", "kmdb_new2all_batch_device", "kmdb_new2all_batch_seq_alphabet_device", "kmdb_node_new2all_batch",
           "kmdb_node_new2all_batch_seq_alphabet", "kmdb_node_new2all_batch_sparse", "kmdbh_query_shard_plan_counts", "kmdbh_query_shard_runs"]
    header = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    L = K.capi.lib()
    for name in new:
        assert name in K.capi.EXPORTS and name + "(" in header and hasattr(L, name), name
    assert K.ABI_VERSION == 8 and L.kmdb_abi_version() == 8 and "#define KMDB_PARTITION_PREFIX_TABLES 2" in header
    assert K.capi.PARTITIONS == ("prefix", "range", "prefix-tables")
    assert ctypes.sizeof(K.capi._NodeStats) == 56


@pytest.mark.parametrize("stem", ["virus_k18", "clade64", "clade64_k25_f01", "synth_k21"])
def test_query_shard_plan_against_numpy(K, golden_dir, stem):
    """kmdbh_query_shard_plan_counts: per shard the kept nodes and own k-mers (as the prefix shards'), the slots of its own bucket table
    (capacities unchanged) and the number of its buckets, against the same computed with numpy from the view."""
    h = K.HostDB(os.path.join(golden_dir, stem + ".db"))
    a = h.view_arrays()
    par, bo, sl = a["parent_id"], a["bucket_offset"], a["slots"]
    P, nb = len(par), len(bo) - 1
    val = (sl >> np.uint64(32)).astype(np.int64)
    cap = np.diff(bo).astype(np.int64)
    bucket = np.repeat(np.arange(nb), cap)
    ok = val != 0x7FFFFFFF
    for S in (1, 2, 3, 8, 11):
        kept, kmers, slots, buckets = h.query_shard_plan_counts(S)
        for s in range(S):
            w = np.bincount(val[ok & (bucket % S == s)], minlength=P)
            keep = w > 0
            for q in range(P - 1, 0, -1):
                if keep[q] and par[q] >= 0:
                    keep[par[q]] = True
            assert int(kept[s]) == int(keep.sum()) and int(kmers[s]) == int(w.sum()), (stem, S, s)
            assert int(slots[s]) == int(cap[s::S].sum()), (stem, S, s)
            assert int(buckets[s]) == max(0, -(-(nb - s) // S)) == len(cap[s::S]), (stem, S, s)
        assert int(slots.sum()) == sl.size and int(kmers.sum()) == int(ok.sum()) and int(buckets.sum()) == nb
    kept1, kmers1 = h.shard_plan_counts(3)
    kept3 = h.query_shard_plan_counts(3)
    assert np.array_equal(kept1, kept3[0]) and np.array_equal(kmers1, kept3[1])


def test_query_shard_plan_needs_the_hashtables(K, golden_dir):
    with pytest.raises(K.KmdbError, match="no hashtables"):
        K.HostDB(os.path.join(golden_dir, "clade64.db"), skip_hashtables=True).query_shard_plan_counts(2)
    with pytest.raises(K.KmdbError, match="shards"):
        K.HostDB(os.path.join(golden_dir, "clade64.db")).query_shard_plan_counts(5000)


def test_kmer_queries_are_cut_at_the_bucket_boundaries(K, golden_dir):
    """kmdbh_query_shard_runs, the split the node driver sends k-mer queries by: the runs of a shard hold exactly the k-mers of its buckets,
    they are ascending, maximal and disjoint, and over all shards they cover the query once — every k-mer crosses PCIe once."""
    q = np.load(os.path.join(golden_dir, "clade64.queries.npz"))
    rng = np.random.default_rng(5)
    queries = [K.sort_unique(q[k]) for k in sorted(q.files, key=lambda s: int(s[1:]))][:6]
    queries += [np.zeros(0, np.uint64), np.array([7], np.uint64), np.array([1, 2, 3, (255 << 32) | 12345, (0xFFFFFFFF << 32) | 1, 0xFFFFFFFFFFFFFFFF], np.uint64),
                K.sort_unique(rng.integers(0, 1 << 40, 5000, dtype=np.uint64)), K.sort_unique(rng.integers(0, 1 << 62, 5000, dtype=np.uint64) << np.uint64(2))]
    for kmers in queries:
        bucket = (kmers >> np.uint64(32)).astype(np.uint64)
        for S in (1, 2, 3, 8, 11):
            seen = np.zeros(kmers.size, np.int32)
            for s in range(S):
                runs = K.capi.query_shard_runs(kmers, S, s)
                own = np.nonzero(bucket % np.uint64(S) == s)[0]
                got = np.concatenate([np.arange(b, e) for b, e in runs]) if runs else np.zeros(0, np.int64)
                assert np.array_equal(got, own), (S, s)
                assert all(b < e for b, e in runs) and all(runs[i][1] < runs[i + 1][0] for i in range(len(runs) - 1))     # ordered, maximal
                for b, e in runs:
                    seen[b:e] += 1
            assert (seen == 1).all()
        assert K.capi.query_shard_runs(kmers, 1, 0) == ([(0, kmers.size)] if kmers.size else [])


def test_cli_gpus_on_the_query_modes(golden_dir):
    db, out = os.path.join(golden_dir, "virus_k18.db"), os.path.join(golden_dir, "o_qs.csv")
    for args in (["new2all", "-gpus", "0", db, db, out], ["one2all", "-gpus", "x", db, db, out]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "ERROR: -gpus expects a number of prefix-bucket shards" in r.stderr, (args, r.stderr)
    r = subprocess.run([EXE, "distance", "-gpus", "2", "jaccard", db, out], capture_output=True, text=True)
    assert r.returncode != 0 and "-gpus applies to all2all, all2all-sp, all2all-parts, new2all and one2all" in r.stderr
    r = subprocess.run([EXE, "new2all", "-gpus", "2", "-partition", "range", db, db, out], capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR: -partition applies to all2all and all2all-sp" in r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert "new2all / one2all: -gpus <N>" in r.stderr


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _dev_rows(torch, dev, nq, N):
    return torch.zeros((max(nq, 1), max(N, 1)), dtype=torch.int32, device=torch.device("cuda", dev))


def _host(torch, buf, nq, N):
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)[:nq, :N].copy()


def _virus_texts(golden_dir, list_name, limit):
    texts = []
    with open(os.path.join(golden_dir, list_name)) as f:
        entries = [ln.strip() for ln in f if ln.strip()]
    for e in entries[:limit]:
        raw = open(os.path.join(golden_dir, e + ".fasta")).read()
        recs = [r.split("\n", 1)[1] if "\n" in r else "" for r in raw.split(">") if r]
        texts.append("\n".join(r.replace("\n", "").replace("\r", "") for r in recs))
    return texts


def _queries(K, golden_dir, h):
    """clade64.queries.npz and the edge cases of test_new2all_bit_exact (an empty query, absent k-mers, a single k-mer, a k-mer of a bucket
    beyond n_buckets); for the virus databases also k-mers of their own genomes, so that the rows are not all zero"""
    q = np.load(os.path.join(golden_dir, "clade64.queries.npz"))
    qs = [K.sort_unique(q[k]) for k in sorted(q.files, key=lambda s: int(s[1:]))]
    qs += [np.zeros(0, np.uint64), np.array([1, 2, 3, (255 << 32) | 12345], np.uint64), qs[0][:1],
           np.array([5, (0xFFFFFFF0 << 32) | 9, 0xFFFFFFFFFFFFFFFF], np.uint64)]
    if h.alphabet == 0 and os.path.exists(os.path.join(golden_dir, "virus.seqs.list")):
        for t in _virus_texts(golden_dir, "virus.seqs.list", 4):
            qs.append(K.sort_unique(np.concatenate([K.extract_kmers(rec, h.k, h.fraction) for rec in t.split("\n")])))
    return qs


@pytest.mark.gpu
@pytest.mark.parametrize("stem,shards", [("clade64", 3), ("virus_k18", 2), ("virus_k18", 8), ("virus_k24", 5)])
def test_query_shard_handles_sum_to_the_whole_database(K, O, golden_dir, dev, stem, shards):
    """kmdb_db_upload_query_shard: every shard holds a pruned tree (n_patterns < P) and only the slots of its own buckets (device_bytes below
    the with-tables upload of the whole database, h2d_bytes = what the plan says); the rows of the shards, ADDED into one device buffer
    (kmdb_new2all_batch_device), equal the unsharded handle's, the oracle's and the reference's; all2all of the same handles sums to the
    full matrix."""
    import torch
    path = os.path.join(golden_dir, stem + ".db")
    h = K.HostDB(path)
    qs = _queries(K, golden_dir, h)
    whole = K.DeviceDB(h, device=dev, with_hashtables=True)
    exp = whole.new2all(qs)
    whole_stats = whole.stats()
    o = O.OracleDB(path)
    assert np.array_equal(exp, np.stack([o.one2all(x) for x in qs]))
    if stem == "clade64":
        ref = np.fromfile(os.path.join(golden_dir, "clade64.n2a.ref.u32"), dtype=np.uint32).reshape(-1, whole.N)
        assert np.array_equal(exp[: ref.shape[0]], ref)
    full = whole.all2all_dense()
    kept, kmers, slots, buckets = h.query_shard_plan_counts(shards)
    buf = _dev_rows(torch, dev, len(qs), whole.N)
    acc = np.zeros_like(full)
    parts = np.zeros_like(exp)
    for s in range(shards):
        d = K.DeviceDB(h, device=dev, query_shard=(s, shards))
        st = d.stats()
        assert 0 < st["n_patterns"] < d.P and st["n_patterns"] == int(kept[s])
        assert st["device_bytes"] < whole_stats["device_bytes"] and st["h2d_bytes"] < whole_stats["h2d_bytes"]
        # what crossed PCIe for the tables: the shard's own slots and its own bucket offsets, nothing of a foreign bucket
        tree_only = K.DeviceDB(h, device=dev, prefix_shard=(s, shards))
        assert st["h2d_bytes"] == tree_only.stats()["h2d_bytes"] + 8 * int(slots[s]) + 8 * (int(buckets[s]) + 1)
        tree_only.close()
        d.new2all_device(qs, buf.data_ptr())
        one = d.new2all(qs)                                       # the host entry on a shard: its own rows alone
        parts += one
        assert int(one.astype(np.uint64).sum()) <= int(exp.astype(np.uint64).sum())
        acc += d.all2all_dense()
        d.close()
    assert np.array_equal(_host(torch, buf, len(qs), whole.N), exp)
    assert np.array_equal(parts, exp)
    assert np.array_equal(acc, full)
    # the device entry on the unsharded handle: adds into the buffer as well (twice the rows now)
    whole.new2all_device(qs, buf.data_ptr())
    assert np.array_equal(_host(torch, buf, len(qs), whole.N), exp * np.uint32(2))
    whole.close()
    with pytest.raises(K.KmdbError, match="no hashtables"):
        K.DeviceDB(K.HostDB(path, skip_hashtables=True), device=dev, query_shard=(0, 2))
    with pytest.raises(K.KmdbError, match="shard_index >= shard_count"):
        K.DeviceDB(h, device=dev, query_shard=(2, 2))
    # db2db needs the pattern ids of the view: a query shard (its slots hold its own DFS indices) is refused, in either position
    part = K.DeviceDB(h, device=dev, query_shard=(0, 2))
    full_t = K.DeviceDB(h, device=dev, with_hashtables=True)
    for a, b in ((part, full_t), (full_t, part)):
        with pytest.raises(K.KmdbError, match="a query shard holds only its own buckets"):
            a.db2db(b)
    part.close()
    full_t.close()


@pytest.mark.gpu
def test_query_shard_count_one_and_a_shard_without_kmers(K, O, golden_dir, dev):
    """shard_count == 1 is the plain upload with tables; a shard that owns no k-mer (more shards than buckets) is a valid handle that
    answers zero rows and a zero matrix."""
    path = os.path.join(golden_dir, "clade64.db")
    h = K.HostDB(path)
    qs = _queries(K, golden_dir, h)[:8]
    whole = K.DeviceDB(h, device=dev, with_hashtables=True)
    exp = whole.new2all(qs)
    one = K.DeviceDB(h, device=dev, query_shard=(0, 1))
    assert np.array_equal(one.new2all(qs), exp) and one.stats()["device_bytes"] == whole.stats()["device_bytes"]
    one.close()
    nb = int(h.view_arrays()["n_buckets"])
    S = nb + 3
    kept, kmers, slots, buckets = h.query_shard_plan_counts(S)
    assert int(kmers[S - 1]) == 0 and int(slots[S - 1]) == 0 and int(buckets[S - 1]) == 0
    empty = K.DeviceDB(h, device=dev, query_shard=(S - 1, S))
    assert not empty.new2all(qs).any() and not empty.all2all_dense().any()
    texts = ["ACGT" * 200, ""]
    rows, cnt = empty.new2all_seq(texts)
    assert not rows.any() and not cnt.any()
    empty.close()
    whole.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stem,k,fraction", [("virus_k18_part1", 18, 1.0), ("virus_k25_f01_part1", 25, 0.1)])
def test_sequence_entry_on_query_shards(K, golden_dir, dev, stem, k, fraction):
    """kmdb_new2all_batch_seq_alphabet_device on 3 query shards: every shard keeps the positions of its own buckets before it sorts; the summed
    rows equal the unsharded device path and the host loader, the summed out_kmer_counts the host loader's counts."""
    import torch
    path = os.path.join(golden_dir, stem + ".db")
    h = K.HostDB(path)
    texts = _virus_texts(golden_dir, "virus.seqs.part2.list", 12)
    texts += [texts[0].lower().replace("t", "u"), texts[1][:500] + "N" + texts[1][500:], "ACGT", "", "A" * (k - 1) + "\n" + "C" * (k - 1)]
    host = []
    for t in texts:
        parts = [K.extract_kmers(rec, k, fraction) for rec in t.split("\n")] if t else []
        host.append(K.sort_unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64))
    whole = K.DeviceDB(h, device=dev, with_hashtables=True)
    exp, cnt = whole.new2all_seq(texts, fraction=fraction)
    assert [int(c) for c in cnt] == [x.size for x in host] and np.array_equal(exp, whole.new2all(host)) and exp.any()
    # the device entry on the unsharded handle
    buf = _dev_rows(torch, dev, len(texts), whole.N)
    cnt_dev = whole.new2all_seq_device(texts, buf.data_ptr(), fraction=fraction)
    assert np.array_equal(_host(torch, buf, len(texts), whole.N), exp) and np.array_equal(cnt_dev, cnt)
    whole.close()
    S = 3
    buf.zero_()
    total = np.zeros(len(texts), np.uint64)
    for s in range(S):
        d = K.DeviceDB(h, device=dev, query_shard=(s, S))
        c = d.new2all_seq_device(texts, buf.data_ptr(), fraction=fraction)
        own = [int((((x >> np.uint64(32)) % np.uint64(S)) == s).sum()) for x in host]
        assert [int(v) for v in c] == own, s                      # unique k-mers of the shard's own buckets
        total += c
        d.close()
    assert np.array_equal(_host(torch, buf, len(texts), whole.N), exp)
    assert np.array_equal(total, cnt)


@pytest.mark.gpu
def test_protein_database_on_query_shards(K, O, golden_dir, dev):
    import torch
    path = os.path.join(golden_dir, "protein_aa.db")
    h = K.HostDB(path)
    with lzma.open(os.path.join(ROOT, "tests", "golden", "protein.aa_100x1000.fasta.xz")) as f:
        recs = O._split_records(f.read())
    texts = [s for _, s in recs[:24]]
    texts += [texts[0].lower(), texts[1][:200] + b"X" + texts[1][200:], texts[2] + b"\n" + texts[3], b"ACDEF", b""]
    want = [O.sort_unique(np.concatenate([O.extract_seq_alphabet(r, h.k, "aa") for r in t.split(b"\n")])) if t else np.zeros(0, np.uint64) for t in texts]
    o = O.OracleDB(path)
    exp = np.stack([o.one2all(w) for w in want])
    buf = _dev_rows(torch, dev, len(texts), h.N)
    total = np.zeros(len(texts), np.uint64)
    for s in range(2):
        d = K.DeviceDB(h, device=dev, query_shard=(s, 2))
        total += d.new2all_seq_device(texts, buf.data_ptr(), alphabet=h.alphabet)
        d.close()
    assert np.array_equal(_host(torch, buf, len(texts), h.N), exp) and [int(c) for c in total] == [w.size for w in want]
    nd = K.NodeDB(h, 2, [dev], partition="prefix-tables")
    rows, cnt = nd.new2all_seq(texts, alphabet=h.alphabet)
    assert np.array_equal(rows, exp) and np.array_equal(cnt, total)
    nd.close()


def _same_rows(sp, dense):
    for i in range(dense.shape[0]):
        c, v = sp.row(i)
        nz = np.nonzero(dense[i])[0]
        assert np.array_equal(c, nz) and np.array_equal(v, dense[i][nz])


@pytest.mark.gpu
@pytest.mark.parametrize("shards,force_rccl", [(3, False), (8, False), (2, True)])
def test_node_driver_new2all(K, O, golden_dir, dev, shards, force_rccl, monkeypatch):
    """kmdb_node_new2all_* on a node uploaded with query shards, over the devices the box has (one: the shards add into the device's buffer in
    turn; with KMDB_NODE_FORCE_RCCL=1 the reduce-scatter runs on a one-rank communicator): dense, sequence and sparse rows equal the
    single-device results, two calls with different nq (the buffer grows), all2all of the same node equals the oracle."""
    if force_rccl:
        monkeypatch.setenv("KMDB_NODE_FORCE_RCCL", "1")
    path = os.path.join(golden_dir, "virus_k18_part1.db")
    h = K.HostDB(path)
    devices = list(range(min(K.device_count(), shards)))
    if force_rccl:
        devices = [dev]
    texts = _virus_texts(golden_dir, "virus.seqs.part2.list", 10) + ["ACGT", ""]
    host = []
    for t in texts:
        parts = [K.extract_kmers(rec, h.k, h.fraction) for rec in t.split("\n")] if t else []
        host.append(K.sort_unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64))
    host.append(np.array([1, 2, 3, (255 << 32) | 12345, (0xFFFFFFF0 << 32) | 9], np.uint64))
    d1 = K.DeviceDB(h, device=dev, with_hashtables=True)
    exp = d1.new2all(host)
    exp_seq, exp_cnt = d1.new2all_seq(texts)
    o = O.OracleDB(path)
    assert np.array_equal(exp[:3], np.stack([o.one2all(x) for x in host[:3]])) and exp.any()
    nd = K.NodeDB(h, shards, devices, partition="prefix-tables")
    st = nd.stats()
    assert st["partition"] == "prefix-tables" and st["n_shards"] == shards and st["n_devices"] == min(shards, len(devices))
    kept, kmers, slots, buckets = h.query_shard_plan_counts(shards)
    assert sum(x["n_patterns"] for x in st["devices"]) == int(kept.sum())
    assert np.array_equal(nd.new2all(host[:2]), exp[:2])              # a small call first: the next one needs a larger buffer
    assert np.array_equal(nd.new2all(host), exp)
    st = nd.stats()
    assert st["call_ms"] > 0 and all(x["call_ms"] > 0 for x in st["devices"])
    assert (st["rccl_version"] > 0) == (st["n_devices"] > 1 or force_rccl)
    if force_rccl:
        assert st["collective_ms"] > 0
    rows, cnt = nd.new2all_seq(texts)
    assert np.array_equal(rows, exp_seq) and np.array_equal(cnt, exp_cnt)
    rows, cnt = nd.new2all_seq(texts[:3])
    assert np.array_equal(rows, exp_seq[:3]) and np.array_equal(cnt, exp_cnt[:3])
    _same_rows(nd.new2all_sparse(host), exp)
    assert nd.new2all([]).shape == (0, h.N)
    assert np.array_equal(nd.all2all_dense(), o.all2all_dense())
    a, b = K.DeviceDB(h, device=dev).all2all_sparse(), nd.all2all_sparse()
    assert a.nnz == b.nnz and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
    assert np.array_equal(nd.new2all(host), exp)                      # and queries again after all2all
    nd.close()
    d1.close()


@pytest.mark.gpu
def test_node_new2all_needs_query_shards(K, golden_dir, dev):
    h = K.HostDB(os.path.join(golden_dir, "clade64.db"))
    q = [np.array([1, 2, 3], np.uint64)]
    for partition in ("prefix", "range"):
        nd = K.NodeDB(h, 2, [dev], partition=partition)
        for call in (lambda: nd.new2all(q), lambda: nd.new2all_seq(["ACGT" * 20]), lambda: nd.new2all_sparse(q)):
            with pytest.raises(K.KmdbError, match="uploaded with partition %s; new2all needs .*prefix-tables" % partition):
                call()
        nd.close()
    with pytest.raises(K.KmdbError, match="need the hashtables"):
        K.NodeDB(K.HostDB(os.path.join(golden_dir, "clade64.db"), skip_hashtables=True), 2, [dev], partition="prefix-tables")
    nd = K.NodeDB(h, 1, [dev], partition="prefix-tables")             # one shard: the plain upload with tables
    d1 = K.DeviceDB(h, device=dev, with_hashtables=True)
    qs = _queries(K, golden_dir, h)[:5]
    assert np.array_equal(nd.new2all(qs), d1.new2all(qs))
    nd.close()
    d1.close()


@pytest.mark.gpu
def test_node_new2all_synthetic_scale(K, O, dev, tmp_path):
    """The shape of test_new2all_thousand_queries_vs_ten_thousand_samples (fresh strains of known clades against a k = 18 database), samples
    and queries cut so that the oracle checks every row in seconds: 4 query shards, batches of 256, k-mer and sequence entry."""
    import importlib
    import torch
    S = importlib.import_module("kmerdb_amd.synth")
    N, cs, L, k, NQ = 2500, 50, 600, 18, 600
    device = torch.device("cuda", dev)
    g, pat = S.synth_database(N, cs, L, k=k, seed=41, device=device)
    arr = S.to_view_arrays(pat)
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"], bucket_offset=tables[0], slots=tables[1])
    devices = list(range(min(K.device_count(), 4)))
    nd = K.NodeDB(view, 4, devices, partition="prefix-tables")
    g_more = S.CladeGenomes(N + NQ, cs, L, seed=41, device=device)
    codes = [g_more.sample(N + i) for i in range(NQ)]
    qs = [S.kmers_of(c, k).cpu().numpy().view(np.uint64) for c in codes]
    got = np.concatenate([nd.new2all(qs[b: b + 256]) for b in range(0, NQ, 256)])
    path = str(tmp_path / "s.db")
    S.write_db(path, k, 1.0, [g.name(i) for i in range(N)], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables)
    o = O.OracleDB(path)
    exp = np.stack([o.one2all(q) for q in qs])
    assert np.array_equal(got, exp) and int(exp.sum()) > 0
    texts = ["".join("ACGT"[int(x)] for x in c.cpu().numpy()) for c in codes]
    seq = [nd.new2all_seq(texts[b: b + 256]) for b in range(0, NQ, 256)]
    assert np.array_equal(np.concatenate([r for r, _ in seq]), exp)
    assert np.array_equal(np.concatenate([c for _, c in seq]), np.array([q.size for q in qs], dtype=np.uint64))
    nd.close()


def _cli(*args):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def _same(a, b):
    assert open(a, "rb").read() == open(b, "rb").read(), (a, b)


@pytest.mark.gpu
def test_cli_query_modes_over_gpus_byte_identical_to_reference_goldens(golden_dir, dev, tmp_path):
    """`new2all -gpus N` / `one2all -gpus N`: the reference's golden tables, byte for byte, through the node driver and query shards"""
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    cwd = os.getcwd()
    os.chdir(golden_dir)          # list entries are ./test/virus/data/<name>
    try:
        r = _cli("new2all", "-gpus", "2", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("n2a.csv")); _same(t("n2a.csv"), g("virus.k18.n2a.csv"))
        assert "2 shards on" in r.stderr and "partition: prefix-tables" in r.stderr
        _cli("new2all", "-sparse", "-gpus", "3", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("n2a.sp.csv")); _same(t("n2a.sp.csv"), g("virus.k18.n2a.sparse.csv"))
        _cli("new2all", "-gpus", "5", g("virus_k18.db"), g("virus.seqs.list"), t("n2a.it.csv")); _same(t("n2a.it.csv"), g("virus.k18.n2a.itself.csv"))
        _cli("new2all", "-host-extract", "-gpus", "3", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("n2a.h.csv")); _same(t("n2a.h.csv"), g("virus.k18.n2a.csv"))
        _cli("new2all", "-host-extract", "-sparse", "-gpus", "1", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("n2a.h1.csv")); _same(t("n2a.h1.csv"), g("virus.k18.n2a.sparse.csv"))
        with open(t("synth.list"), "w") as f:
            f.write(g("synth.synth") + "\n")
        _cli("new2all", "-multisample-fasta", "-gpus", "2", g("synth_k21.db"), t("synth.list"), t("n2a")); _same(t("n2a"), g("synth.n2a"))
        _cli("new2all", "-multisample-fasta", "-sparse", "-gpus", "5", g("synth_k21.db"), t("synth.list"), t("n2a-sp")); _same(t("n2a-sp"), g("synth.n2a-sparse"))
        _cli("new2all", "-multisample-fasta", "-sparse", "-gpus", "3", "-max", "69", "-min", "num-kmers:21", g("synth_k21.db"), t("synth.list"), t("n2a-mm"))
        _same(t("n2a-mm"), g("synth.n2a.sparse.above-below"))
        r = _cli("one2all", "-gpus", "3", g("virus_k25_f01_part1.db"), "./test/virus/data/MT159713", t("MT159713.csv"))
        _same(t("MT159713.csv"), g("virus.MT159713.csv"))
        assert "3 shards on" in r.stderr
    finally:
        os.chdir(cwd)
    # a protein database through the front-end: one2all of a record that is a sample, sharded and not
    with lzma.open(os.path.join(ROOT, "tests", "golden", "protein.aa_100x1000.fasta.xz")) as f:
        first = f.read().split(b">")[6]
    (tmp_path / "q.fasta").write_bytes(b">" + first)
    _cli("one2all", g("protein_aa.db"), t("q.fasta"), t("aa.csv"))
    _cli("one2all", "-gpus", "2", g("protein_aa.db"), t("q.fasta"), t("aa.g2.csv"))
    _same(t("aa.g2.csv"), t("aa.csv"))
