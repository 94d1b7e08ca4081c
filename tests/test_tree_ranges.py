"""Tree ranges: the second partition of a database over the GPUs of a node (host_ranges.cpp, kmdb_db_upload_range,
kmdb_node_upload_partition, `-gpus N -partition range`).  The CPU tests check the plan against numpy and the sum of the ranges on the
oracle; the GPU tests mirror the prefix-shard tests of test_gpu_parity.py on the same databases and references."""
import ctypes
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

MAX_SHARDS = 4096                                               # KMDB_MAX_SHARDS (csrc/kmdb_internal.h)


@pytest.fixture(scope="module")
def S(K):
    return importlib.import_module("kmerdb_amd.synth")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


def _preorder(par):
    """DFS pre-order position and depth of every node from parent_id alone, by the device layout's convention: the children of a node,
    and the roots, in ascending pattern id (parent_id[p] < p)."""
    P = len(par)
    size = np.ones(P, np.int64)
    for p in range(P - 1, -1, -1):
        if par[p] >= 0:
            size[par[p]] += size[p]
    pre, depth, nxt = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)
    root_next = 0
    for p in range(P):
        q = int(par[p])
        if q < 0:
            pre[p], depth[p] = root_next, 1
            root_next += size[p]
        else:
            pre[p], depth[p] = nxt[q], depth[q] + 1
            nxt[q] += size[p]
        nxt[p] = pre[p] + 1
    assert P == 0 or sorted(pre.tolist()) == list(range(P))
    return pre, depth


def _check_plan(par, plan, R):
    """the conditions every range plan meets, exactly (no tolerance: none of this is a measurement)"""
    P = len(par)
    pre, depth = _preorder(par)
    kept, own, first_depth, rof = (plan[k].astype(np.int64) for k in ("kept", "own", "first_depth", "range_of"))
    assert len(kept) == len(own) == len(first_depth) == R and len(rof) == P
    assert int(own.sum()) == P and (P == 0 or (0 <= rof.min() and rof.max() < R))
    assert np.array_equal(np.bincount(rof, minlength=R), own)
    # contiguous in the pre-order, and in order: the ranges read along the pre-order never go back
    order = np.argsort(pre)
    assert np.all(np.diff(rof[order]) >= 0)
    for s in range(R):
        if own[s] == 0:
            assert kept[s] == 0 and first_depth[s] == 0
            continue
        first = order[int(own[:s].sum())]
        assert rof[first] == s and first_depth[s] == depth[first]
        assert kept[s] == own[s] + first_depth[s] - 1
        # what the formula counts: the ancestors of the range's nodes that lie outside it are the ancestors of its first node
        if R <= 11:
            members = np.nonzero(rof == s)[0]
            anc = set()
            for p in members:
                q = int(par[p])
                while q >= 0 and q not in anc:
                    anc.add(q)
                    q = int(par[q])
            outside = {q for q in anc if rof[q] != s}
            chain, q = set(), int(par[first])
            while q >= 0:
                chain.add(q)
                q = int(par[q])
            assert outside == chain and len(chain) == first_depth[s] - 1
    ne = own > 0
    assert int(kept.sum()) == P + int((first_depth[ne] - 1).sum())
    return pre, depth


@pytest.mark.parametrize("stem", ["virus_k18", "clade64", "clade64_k25_f01", "synth_k21"])
def test_range_plan_against_numpy(K, golden_dir, stem):
    """kmdbh_range_plan on databases loaded WITHOUT their hashtables: ranges contiguous in the pre-order recomputed from parent_id, every
    pattern in one range, kept = own + depth(first) - 1, sum(kept) = P + sum(depth(first) - 1); a pure function of (view, R)."""
    h = K.HostDB(os.path.join(golden_dir, stem + ".db"), skip_hashtables=True)
    a = h.view_arrays()
    assert a["n_buckets"] == 0
    par = a["parent_id"]
    P = len(par)
    for R in (1, 2, 3, 8, 11, P + 5):
        if R > MAX_SHARDS:
            with pytest.raises(K.KmdbError, match="ranges"):
                h.range_plan(R)
            continue
        plan = h.range_plan(R)
        _check_plan(par, plan, R)
        again = h.range_plan(R)
        for k in plan:
            assert np.array_equal(plan[k], again[k]), k
        if R == 1:
            assert plan["kept"][0] == P and plan["first_depth"][0] == 1
        # balanced by the cost estimate: no range above its share by more than the dearest node
        cost = plan["cost"].astype(np.int64)
        assert int(cost.sum()) > 0 and (R > P or int(cost.max()) > 0)
    # the same plan from the view that carries the hashtables: they are not read
    h2 = K.HostDB(os.path.join(golden_dir, stem + ".db"))
    for k, v in h2.range_plan(8).items():
        assert np.array_equal(v, h.range_plan(8)[k]), k


def test_range_plan_on_small_forests(K):
    """more ranges than patterns, one pattern, no pattern, one sample, a forest of roots only, a chain: legal inputs, empty ranges"""
    z32 = lambda n: np.zeros(n, np.uint32)      # noqa: E731
    cases = [np.array([-1], np.int64), np.zeros(0, np.int64), np.full(7, -1, np.int64), np.arange(-1, 9, dtype=np.int64),
             np.array([-1, 0, 0, 1, -1, 4, 1, 2, 4, 0], np.int64)]
    for par in cases:
        P = len(par)
        for N in (1, 3):
            view = K.make_view(18, N, np.ones(P, np.int64), par, np.minimum(np.arange(P) % 3 + 1, N).astype(np.uint32), z32(P), z32(P), z32(P),
                               np.zeros(P, np.uint64), np.zeros(1, np.uint64))
            for R in (1, 2, 5, P + 5):
                plan = K.range_plan(ctypes.pointer(view[0]), R)
                _check_plan(par, plan, R)
                assert np.count_nonzero(plan["own"]) <= max(P, 0)
    # the pre-order itself on the last forest: range_of with one range per node is the position
    par = cases[-1]
    view = K.make_view(18, 3, np.ones(10, np.int64), par, np.ones(10, np.uint32), z32(10), z32(10), z32(10), np.zeros(10, np.uint64), np.zeros(1, np.uint64))
    plan = K.range_plan(ctypes.pointer(view[0]), 10)
    pre, _ = _preorder(par)
    assert list(pre) == [0, 1, 4, 2, 7, 8, 3, 5, 9, 6]             # by hand: 0 (1 (3 6) 2 (7) 9) 4 (5 8)
    if np.all(plan["own"] == 1):                                # (equal costs: every node its own range)
        assert np.array_equal(plan["range_of"], pre)


def _range_view_arrays(arr, keep, num_kmers):
    """the view arrays of the kept nodes alone: parents re-indexed among them, streams packed again"""
    idx = np.nonzero(keep)[0]
    new = np.full(len(keep), -1, np.int64)
    new[idx] = np.arange(len(idx))
    par = arr["parent_id"][idx]
    out = {"num_kmers": num_kmers[idx].astype(np.int64), "parent_id": np.where(par < 0, -1, new[np.maximum(par, 0)]).astype(np.int64)}
    assert np.all((par < 0) | (out["parent_id"] >= 0))          # a kept node's parent is kept
    for k in ("num_samples", "num_local", "last_sample_id", "num_bits"):
        out[k] = arr[k][idx]
    words = (arr["num_bits"][idx].astype(np.int64) + 127) // 128 * 2      # streams are padded to 128 bits (reference src/pattern.h:79-81)
    data, offs, pos = [], [], 0
    for p, n in zip(idx, words):
        lo = int(arr["data_offset"][p])
        offs.append(pos)
        data.append(arr["data"][lo:lo + int(n)])
        pos += int(n)
    out["data_offset"] = np.array(offs, np.uint64)
    out["data"] = np.concatenate(data + [np.zeros(2, np.uint64)]).astype(np.uint64)
    return out


def test_tree_ranges_sum_to_full_matrix_on_the_oracle(S, O, K):
    """Every range written as a database of its kept nodes (the ancestors before the range at num_kmers = 0): the oracle's matrices of the
    ranges sum to its matrix of the whole database."""
    N, cs, L, k = 32, 8, 6000, 18
    g, pat = S.synth_database(N, cs, L, k=k, seed=11)
    arr = S.to_view_arrays(pat)
    names = [g.name(i) for i in range(N)]
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"],
                       arr["num_bits"], arr["data_offset"], arr["data"])
    P = len(arr["parent_id"])
    with tempfile.TemporaryDirectory() as td:
        S.write_db(os.path.join(td, "f.db"), k, 1.0, names, pat["sample_counts"], arr)
        ref = O.OracleDB(os.path.join(td, "f.db"), skip_hashtables=True).all2all_dense()
        assert int(ref.astype(np.uint64).sum()) > 0
        for R in (2, 3, 8):
            plan = K.range_plan(ctypes.pointer(view[0]), R)
            pre, _ = _check_plan(arr["parent_id"], plan, R)
            rof = plan["range_of"].astype(np.int64)
            acc = np.zeros_like(ref)
            total_kept = 0
            for s in range(R):
                own = rof == s
                keep = own.copy()
                members = np.nonzero(own)[0]
                for p in members[np.argmin(pre[members])][None] if len(members) else []:      # the ancestors of the range's first node
                    q = int(arr["parent_id"][p])
                    while q >= 0:
                        keep[q] = True
                        q = int(arr["parent_id"][q])
                assert int(keep.sum()) == int(plan["kept"][s])
                total_kept += int(keep.sum())
                sub = _range_view_arrays(arr, keep, np.where(own, arr["num_kmers"], 0))
                path = os.path.join(td, "r%d_%d.db" % (R, s))
                S.write_db(path, k, 1.0, names, pat["sample_counts"], sub)
                acc += O.OracleDB(path, skip_hashtables=True).all2all_dense()
            assert np.array_equal(acc, ref), R
            assert P <= total_kept == int(plan["kept"].sum())


def test_range_plan_arguments(K, golden_dir):
    """no ranges, too many, null pointers, a parent that does not precede its child: an error with a message, nothing leaves the C boundary"""
    h = K.HostDB(os.path.join(golden_dir, "synth_k21.db"), skip_hashtables=True)
    with pytest.raises(K.KmdbError, match="no ranges"):
        h.range_plan(0)
    with pytest.raises(K.KmdbError, match="more than %d ranges" % MAX_SHARDS):
        h.range_plan(MAX_SHARDS + 1)
    assert len(h.range_plan(MAX_SHARDS)["kept"]) == MAX_SHARDS
    L = K.lib()
    buf = np.zeros(4, np.uint64)
    for args in ((None, 2, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data), (h.view, 2, None, buf.ctypes.data, buf.ctypes.data),
                 (h.view, 2, buf.ctypes.data, None, buf.ctypes.data), (h.view, 2, buf.ctypes.data, buf.ctypes.data, None)):
        assert L.kmdbh_range_plan(*args, None, None) != 0
        assert b"null argument" in L.kmdb_last_error()
    assert L.kmdbh_range_plan(h.view, 2, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None) == 0      # range_of / first_depth may be NULL
    a = h.view_arrays()
    bad = a["parent_id"].copy()
    bad[1] = 3
    view = K.make_view(h.k, h.N, a["num_kmers"], bad, a["num_samples"], a["num_local"], a["last_sample_id"], a["num_bits"], a["data_offset"], a["data"])
    with pytest.raises(K.KmdbError, match="parent_id >= pattern id"):
        K.range_plan(ctypes.pointer(view[0]), 2)
    # the upload's own arguments are checked before any device work (so also on a box without a GPU)
    with pytest.raises(K.KmdbError, match="range_index >= range_count"):
        K.DeviceDB(h, tree_range=(2, 2))
    with pytest.raises(K.KmdbError, match="range_count"):
        K.DeviceDB(h, tree_range=(0, 0))
    with pytest.raises(K.KmdbError, match="range_count"):
        K.DeviceDB(h, tree_range=(0, MAX_SHARDS + 1))
    with pytest.raises(K.KmdbError, match="parent_id >= pattern id"):
        K.DeviceDB(view, tree_range=(0, 2))
    with pytest.raises(ValueError):
        K.DeviceDB(h, tree_range=(0, 2), with_hashtables=True)
    with pytest.raises(ValueError):
        K.NodeDB(h, 2, [0], partition="subtree")
    ptr = ctypes.c_void_p()
    devs = (ctypes.c_int32 * 1)(0)
    assert L.kmdb_node_upload_partition(h.view, 2, devs, 1, 7, ctypes.byref(ptr)) != 0 and b"unknown partition" in L.kmdb_last_error()
    assert L.kmdb_node_upload_partition(h.view, MAX_SHARDS + 1, devs, 1, 1, ctypes.byref(ptr)) != 0 and b"shards" in L.kmdb_last_error()
    assert not ptr.value


def test_abi_8_is_additive(K, golden_dir):
    """ABI 8 added entry points and changed no struct, so a view stamped by a caller compiled against the header of ABI 7 is still served
    (the check comes before any device work); anything older or newer is refused."""
    h = K.HostDB(os.path.join(golden_dir, "synth_k21.db"), skip_hashtables=True)
    a = h.view_arrays()
    assert K.ABI_VERSION == 8 and K.capi._NodeStats.partition.offset == 12 and ctypes.sizeof(K.capi._NodeStats) == 56
    for abi, ok in ((6, False), (7, True), (8, True), (9, False)):
        view = K.make_view(h.k, h.N, a["num_kmers"], a["parent_id"], a["num_samples"], a["num_local"], a["last_sample_id"], a["num_bits"], a["data_offset"], a["data"])
        view[0].abi_version = abi
        if ok:
            assert len(K.range_plan(ctypes.pointer(view[0]), 2)["kept"]) == 2
            if K.device_count() == 0:
                with pytest.raises(K.KmdbError, match="no HIP device"):
                    K.DeviceDB(view)
        else:
            for call in (lambda: K.range_plan(ctypes.pointer(view[0]), 2), lambda: K.DeviceDB(view), lambda: K.DeviceDB(view, tree_range=(0, 2)),
                         lambda: K.NodeDB(view, 2, [0], partition="range")):
                with pytest.raises(K.KmdbError, match="ABI version"):
                    call()


def test_cli_partition_usage_errors(golden_dir):
    exe = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
    db, out = os.path.join(golden_dir, "virus_k18.db"), os.path.join(golden_dir, "o_part.csv")
    for args, msg in ((["all2all", "-gpus", "2", "-partition", "subtree", db, out], "-partition expects prefix or range"),
                      (["all2all", "-partition", "range", db, out], "-partition goes with -gpus"),
                      (["all2all-sp", "-partition", "prefix", db, out], "-partition goes with -gpus"),
                      (["all2all-parts", "-gpus", "2", "-partition", "range", db, out], "-partition applies to all2all and all2all-sp"),
                      (["new2all", "-partition", "range", db, db, out], "-partition applies to all2all and all2all-sp")):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "ERROR: " + msg in r.stderr, (args, r.stderr)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert "-partition prefix|range" in r.stderr


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stem,ranges", [("virus_k18", 2), ("virus_k18", 8), ("clade64", 3), ("virus_k24", 5)])
def test_upload_ranges_of_a_real_db_sum_to_full_matrix(K, golden_dir, dev, stem, ranges):
    """kmdb_db_upload_range on a .db built by the real reference and loaded WITHOUT its hashtables: every range runs the block-record
    pipeline, its matrix sums to its own checksum, holds exactly the nodes the plan says, and the parts sum to the reference's matrix."""
    h = K.HostDB(os.path.join(golden_dir, stem + ".db"), skip_hashtables=True)
    assert h.view_arrays()["n_buckets"] == 0
    ref = np.fromfile(os.path.join(golden_dir, stem + ".a2a.ref.u32"), dtype=np.uint32)
    plan = h.range_plan(ranges)
    acc = np.zeros_like(ref)
    total_pairs, kept = 0, []
    for s in range(ranges):
        d = K.DeviceDB(h, device=dev, tree_range=(s, ranges))
        part = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
        st = d.stats()
        assert st["path"] == K.capi.PATH_RECORDS and (st["n_records"] + st["n_direct"] > 0 or st["sum_pairs"] == 0)
        assert st["n_patterns"] == int(plan["kept"][s]) and 0 < st["n_patterns"] < d.P
        kept.append(st["n_patterns"])
        assert st["sum_pairs"] == int(part.astype(np.uint64).sum())          # the range's own checksum identity
        total_pairs += st["sum_pairs"]
        # slices of the RESIDENT stream work on a range handle as on any other
        if s == ranges - 1:
            sl = sum(d.all2all_dense(shard=(i, 3)).astype(np.uint64) for i in range(3)).astype(np.uint32)
            assert np.array_equal(sl, part)
        acc += part
        d.close()
    assert np.array_equal(acc, ref) and total_pairs == int(ref.astype(np.uint64).sum())
    ne = plan["own"] > 0
    assert sum(kept) == d.P + int((plan["first_depth"][ne].astype(np.int64) - 1).sum())
    # one range of one is the plain upload
    d = K.DeviceDB(h, device=dev, tree_range=(0, 1))
    assert d.stats()["n_patterns"] == d.P and np.array_equal(d.all2all_dense(), ref)
    d.close()


def _same_sparse(a, b):
    assert a.nnz == b.nnz and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)


@pytest.mark.gpu
@pytest.mark.parametrize("stem,shards", [("virus_k18", 3), ("clade64", 8), ("clade64_k25_f01", 2)])
def test_node_driver_with_tree_ranges(K, golden_dir, dev, stem, shards, monkeypatch):
    """kmdb_node_upload_partition(KMDB_PARTITION_RANGE) on a database loaded without hashtables: dense == the reference's (cold and warm),
    sparse and filtered sparse with a measure == the single-device calls, the devices hold the plan's nodes and received the bytes the plan
    says; on the clade databases fewer bytes than the prefix partition of the same count; the same through the one-rank RCCL path."""
    path = os.path.join(golden_dir, stem + ".db")
    h = K.HostDB(path, skip_hashtables=True)
    ref = np.fromfile(os.path.join(golden_dir, stem + ".a2a.ref.u32"), dtype=np.uint32)
    devices = list(range(K.device_count()))
    plan = h.range_plan(shards)
    kept = int(plan["kept"].sum())
    ne = plan["own"] > 0
    cnt = h.sample_kmers.astype(np.uint32)
    d1 = K.DeviceDB(h, device=dev)
    assert kept == d1.P + int((plan["first_depth"][ne].astype(np.int64) - 1).sum())
    one = d1.stats()["h2d_bytes"]
    stream_bytes = one - 32 * d1.P                                    # a whole upload: 24 B of fields + the 8-byte k-mer count per node, and the streams
    sp1 = d1.all2all_sparse()
    flt = [("jaccard", 0.02, None), ("num-kmers", None, 5000.0)]
    spf1 = d1.all2all_sparse_filtered(flt, cnt, measure="mash")
    totals = {}
    for force in ("0", "1"):
        monkeypatch.setenv("KMDB_NODE_FORCE_RCCL", force)
        nd = K.NodeDB(h, shards, devices, partition="range")
        assert np.array_equal(nd.all2all_dense(), ref)
        st = nd.stats()
        assert st["partition"] == "range" and st["n_shards"] == shards and st["n_devices"] == min(shards, len(devices)) and st["call_ms"] > 0
        assert (st["rccl_version"] > 0) == (st["n_devices"] > 1 or force == "1") and st["plan_s"] > 0
        assert np.array_equal(nd.all2all_dense(), ref)                # warm call
        assert sum(x["n_shards"] for x in st["devices"]) == shards
        assert sum(x["n_patterns"] for x in st["devices"]) == kept
        total = sum(x["h2d_bytes"] for x in st["devices"])
        print("%s x %d (rccl %s): kept %d of P %d, h2d %d, whole upload %d" % (stem, shards, force, kept, d1.P, total, one))
        assert 24 * kept < total <= 24 * kept + shards * stream_bytes, (total, one, kept)
        totals[force] = total
        _same_sparse(sp1, nd.all2all_sparse())
        b = nd.all2all_sparse(flt, cnt, measure="mash")
        _same_sparse(spf1, b)
        assert np.array_equal(spf1.measure, b.measure, equal_nan=True)
        nd.close()
    monkeypatch.delenv("KMDB_NODE_FORCE_RCCL")
    assert totals["0"] == totals["1"]
    # prefix buckets on this view still need what it does not carry
    with pytest.raises(K.KmdbError, match="need the hashtables"):
        K.NodeDB(h, 2, devices, partition="prefix")
    if stem.startswith("clade64"):
        # the plan keeps 1.004 x / 1.002 x P here, a prefix shard nearly the whole tree each: fewer bytes over PCIe for the same count
        hp = K.HostDB(path)
        ndp = K.NodeDB(hp, shards, devices)
        stp = ndp.stats()
        prefix_total = sum(x["h2d_bytes"] for x in stp["devices"])
        print("%s x %d: prefix partition h2d %d, nodes %d" % (stem, shards, prefix_total, sum(x["n_patterns"] for x in stp["devices"])))
        assert stp["partition"] == "prefix" and totals["0"] < prefix_total
        ndp.close()
    d1.close()


@pytest.mark.gpu
def test_tree_ranges_of_a_synthetic_database_with_wide_nodes(K, S, dev):
    """3000 samples (wide nodes and the second level in play), 8 ranges: the parts sum to the unsharded matrix of the same engine, and rows of
    the sum agree with the definition |K_i ∩ K_j| recomputed from the k-mer sets."""
    import torch
    from test_gpu_parity import _definition_rows
    N, cs, L, k, R = 3000, 100, 1500, 18, 8
    device = torch.device("cuda", dev)
    g, pat = S.synth_database(N, cs, L, k=k, seed=9, device=device)
    arr = S.to_view_arrays(pat)
    view = K.make_view(k, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    full = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
    assert d.stats()["n_wide"] > 0
    d.close()
    plan = K.range_plan(ctypes.pointer(view[0]), R)
    acc = np.zeros_like(full)
    for s in range(R):
        d = K.DeviceDB(view, device=dev, tree_range=(s, R))
        part = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
        st = d.stats()
        assert st["path"] == K.capi.PATH_RECORDS and st["n_patterns"] == int(plan["kept"][s]) and st["sum_pairs"] == int(part.astype(np.uint64).sum())
        acc += part
        d.close()
    assert np.array_equal(acc, full)
    nd = K.NodeDB(view, R, [dev], partition="range")
    assert np.array_equal(nd.all2all_dense(), full)
    nd.close()
    tri_row = lambda i: acc[i * (i - 1) // 2: i * (i - 1) // 2 + i]      # noqa: E731
    _definition_rows(S, g, k, 1.0, N, cs, (1, cs - 1, cs, N // 2, N - 1), lambda i, cols: tri_row(i)[cols], device)


@pytest.mark.gpu
def test_tree_ranges_of_degenerate_databases(K, S, dev):
    import torch
    z = lambda n: torch.zeros(n, dtype=torch.int64)     # noqa: E731
    # only the empty pattern, one sample (N = 1, P = 1), more ranges than patterns
    pat = {"num_kmers": z(1), "parent": torch.tensor([-1]), "num_samples": z(1), "num_local": z(1), "local_ptr": z(2), "local_ids": z(0)}
    arr = S.to_view_arrays(pat)
    view = K.make_view(18, 1, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    for s in range(3):
        d = K.DeviceDB(view, device=dev, tree_range=(s, 3))
        assert d.all2all_dense().size == 0 and d.all2all_sparse().nnz == 0
        d.close()
    nd = K.NodeDB(view, 3, [dev], partition="range")
    assert nd.all2all_dense().size == 0
    nd.close()
    # three samples, a root over two leaves and a lone root; 9 ranges of 4 patterns: the empty ranges give zero matrices
    pat = {"num_kmers": torch.tensor([3, 5, 7, 9]), "parent": torch.tensor([-1, 0, 0, -1]),
           "num_samples": torch.tensor([2, 3, 3, 1]), "num_local": torch.tensor([2, 1, 1, 1]),
           "local_ptr": torch.tensor([0, 2, 3, 4, 5]), "local_ids": torch.tensor([0, 1, 2, 2, 1])}
    arr = S.to_view_arrays(pat)
    view = K.make_view(18, 3, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"],
                       arr["last_sample_id"], arr["num_bits"], arr["data_offset"], arr["data"])
    d = K.DeviceDB(view, device=dev)
    full = d.all2all_dense()
    d.close()
    assert full.tolist() == [15, 12, 12]                        # cells (1,0), (2,0), (2,1): 3 + 5 + 7 | 5 + 7 | 5 + 7
    for R in (2, 4, 9):
        plan = K.range_plan(ctypes.pointer(view[0]), R)
        acc = np.zeros_like(full)
        for s in range(R):
            d = K.DeviceDB(view, device=dev, tree_range=(s, R))
            part = d.all2all_dense()
            st = d.stats()
            assert st["sum_pairs"] == int(part.sum())
            assert st["n_patterns"] == (int(plan["kept"][s]) if plan["own"][s] else 1)      # an empty range holds pattern 0 at weight 0
            assert plan["own"][s] or not part.any()
            acc += part
            d.close()
        assert np.array_equal(acc, full), R
        nd = K.NodeDB(view, R, [dev], partition="range")
        assert np.array_equal(nd.all2all_dense(), full)
        nd.close()


@pytest.mark.gpu
def test_cli_tree_ranges_byte_identical_to_reference_goldens(golden_dir, dev, tmp_path):
    from test_gpu_parity import _cli, _same
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    for n in ("2", "3", "5"):
        r = _cli("all2all", "-gpus", n, "-partition", "range", g("virus_k18_parts.db"), t("k18.r%s.csv" % n))
        _same(t("k18.r%s.csv" % n), g("virus.k18.csv"))
        assert "loaded without hashtables" in r.stderr and n + " shards on" in r.stderr and "partition: range" in r.stderr
    r = _cli("all2all-sp", "-gpus", "3", "-partition", "range", g("virus_k18.db"), t("k18.sp.r3.csv"))
    _same(t("k18.sp.r3.csv"), g("virus.k18.sparse.csv"))
    assert "loaded without hashtables" in r.stderr
    r = _cli("all2all", "-sparse", "-gpus", "2", "-partition", "range", g("virus_k18_parts.db"), t("k18.r2.sparse.csv"))
    _same(t("k18.r2.sparse.csv"), g("virus.k18.sparse.csv"))
    # the default stays what it was
    r = _cli("all2all", "-gpus", "2", "-partition", "prefix", g("virus_k18_parts.db"), t("k18.p2.csv")); _same(t("k18.p2.csv"), g("virus.k18.csv"))
    assert "sharded by k-mer prefix bucket" in r.stderr and "partition: prefix" in r.stderr
