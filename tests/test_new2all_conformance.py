"""new2all conformance: the branches of csrc/hash_probe.h (kmdb_probe) and csrc/new2all.hip (probe, sort, walk, packed nodes) that the
goldens and the random forests do not aim at, each with a case of tests/new2all_cases.py built around the engine's own thresholds, and
censuses on the host that prove what the cases hold before a device runs.

  P1 .. P4  the probe on FABRICATED tables: capacities 1 and 2, odd table offsets (the scalar path), offsets = 2 mod 4, groups entered in
            the middle (`first`), the wrap from the last group to group 0, an empty slot before `first`, the long way round a table with one
            empty slot, key 0 (an empty slot's key), one key in three buckets, a word beyond the buckets.  The same tables through db2db.
  W1        the queue of long lists: one workgroup files 1023 / 1024 / 1025 / 1500 entries for a query (N2_QCAP = 1024); a full queue
            sends lists of 33 ids to the visiting thread's inline decode, some of them ending at id N - 1.
  W2        the workgroup's stretch of the hit list: `prev` of thread 0, the entry beyond the workgroup, searches that leave the LDS
            stretch, an H that counts the hits of three later workgroups; 511 / 512 / 513 / 1024 / 1025 hit patterns per query.
  W3a, W3b  batch and key geometry: 600 one-hit queries, empty and all-miss queries first, inside and before the last, a query three
            times, P = 2^10 - 1 and 2^10, the last DFS node in the last query, batches of 1, 2, 3, 256 and 257 queries.
  W4_*      N = 11008 | 11009 and 9984 | 9985: the last histogram in LDS and the first in memory at 512 and at 1024 threads.
  W5        packed node records whose list length and run count clip at 0xFFFF (N = 131200).

References: the row from the definition in numpy (new2all_cases.Case.rows), the CPU oracle's one2all on the written file and, where it is
built, the real reference; test_references_agree holds them against each other for every case.  On the device everything is compared
with the definition, bit for bit (uint32 arrays: no tolerance), never with a second run of the engine.  Every case runs under the five
environments of test_kernel_variants.N2A_VARIANTS, W4_* and W5 included (the whole file takes seconds on an MI355X)."""
import os

import numpy as np
import pytest

import conftest
import new2all_cases as C
from gamma_cases import db2db_from_lists
from test_gpu_parity import _Laps
from test_kernel_variants import N2A_VARIANTS, _S, env          # noqa: F401  (env: the fixture)

assert len(N2A_VARIANTS) == 5


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


class _Lap(_Laps):
    def done(self):
        print(self.name + " " + " ".join(self.laps), flush=True)
        super().done()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> the case, written as a .db file once"""
    folder = str(tmp_path_factory.mktemp("new2all"))
    S = _S()

    def get(name):
        c = C.case(name)
        if c.path is None:
            c.write(S, os.path.join(folder, name + ".db"))
        return c
    return get


def _same(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if np.array_equal(got, exp):
        return
    bad = np.argwhere(got != exp)
    first = ["(query %d, sample %d) got %d, expected %d" % (r, c, int(got[r, c]), int(exp[r, c])) for r, c in bad[:3].tolist()]
    pytest.fail("%s: %d of %d cells differ in %d queries; first: %s" % (what, bad.shape[0], exp.size, np.unique(bad[:, 0]).size, "; ".join(first)))


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
def test_references_agree(O, built, tmp_path):
    """the definition in numpy == the CPU oracle's one2all on the written file, every query of every case; == the real reference where it is
    built (the words beyond the buckets are kept from its reader)"""
    ref = O.have_ref()
    for name in C.NAMES:
        c = built(name)
        want = c.rows()
        odb = O.OracleDB(c.path)
        try:
            assert (odb.N, odb.P, odb.n_buckets) == (c.N, c.P, C.N_BUCKETS), name
            got = np.stack([odb.one2all(q) for q in c.queries])
        finally:
            odb.close()
        _same(got, want, "oracle against the definition, case " + name)
        assert want.any(), name
        if ref:
            qs = [C.in_range(c, q) for q in c.queries]
            O.write_kmers_bin(str(tmp_path / "q.bin"), C.K_LEN, 1.0, [("q%d" % i, q) for i, q in enumerate(qs)])
            r, _ = O.ref_one2all(c.path, str(tmp_path / "q.bin"), str(tmp_path / "r.u32"))
            _same(r.reshape(len(qs), c.N), want, "reference against the definition, case " + name)


def test_the_reference_reads_the_fabricated_tables(O, built, tmp_path):
    """tables of one and two slots, filled to the last slot but one, are files the reference's own reader takes (skipped without its build)"""
    conftest.require_ref_or_skip(O.REF_DRIVER, "needs the reference build (oracle/_ref/ref_driver)")
    c = built("P1")
    qs = [C.in_range(c, q) for q in c.queries[:300]]
    O.write_kmers_bin(str(tmp_path / "q.bin"), C.K_LEN, 1.0, [("q%d" % i, q) for i, q in enumerate(qs)])
    r, _ = O.ref_one2all(c.path, str(tmp_path / "q.bin"), str(tmp_path / "r.u32"))
    _same(r.reshape(len(qs), c.N), c.rows()[:300], "reference, case P1")


def test_probe_cases_hold_their_edges():
    """The probe census (new2all_cases.probe_census restates kmdb_probe per queried word).  P1: empty tables of one slot; tables of two
    with the key found at home, an absent key that goes one slot on and one that ends at once; tables of 4 and of 16 on the scalar path
    (odd offset) and on the four-slot path at offsets = 2 mod 4, hits and misses on each, probes that wrap.  P2: all offsets = 0 mod 4;
    per capacity 4 / 16 / 64 keys found at homes = 0, 1, 2, 3 mod 4, keys found in the group after their home group, found after a wrap,
    found although an EMPTY slot lies before `first`, absent keys likewise, absent keys that end one slot behind a full home.  P3: tables
    with one empty slot e = 0 mod 4, a key of home e + 1 found at e - 1 in the last group before the revisit (cap / 4 loads), absent keys
    of homes e + 1 .. e + 3 that end at e on the revisit (cap / 4 + 1 loads), in tables of 16 and of 4.  P4: key 0 found at home, found
    behind another key, missed at an empty home slot between full ones and in an empty table; one key under three patterns in three
    buckets (four tables); words beyond the buckets."""
    pr = {n: [C.probe_census(C.case(n).T, w) for w in C.case(n).about["probes"]] for n in C.PROBE}
    has = lambda n, **kw: sum(all(x.get(k) == v for k, v in kw.items()) for x in pr[n])          # noqa: E731
    # P1
    assert tuple(C.case("P1").T.caps[:9]) == (1, 16, 1, 4, 2, 8, 2, 2, 16)
    assert has("P1", cap=1, found=False, steps=1) >= 80 and has("P1", cap=1, found=True) == 0
    assert has("P1", cap=2, found=True, steps=1) >= 60 and has("P1", cap=2, found=False, steps=2) >= 60 and has("P1", cap=2, found=False, steps=1) >= 60
    for cap in (4, 16):
        for found in (True, False):
            assert has("P1", cap=cap, path="scalar", found=found) >= 20, (cap, found)
            assert sum(x.get("cap") == cap and x["path"] == "four" and x["off"] % 4 == 2 and x["found"] == found for x in pr["P1"]) >= 20, (cap, found)
            assert has("P1", cap=cap, path="scalar", found=found, wrapped=True) >= 5 and has("P1", cap=cap, path="four", found=found, wrapped=True) >= 5
    assert all(x["path"] == "scalar" for x in pr["P1"] if x["cap"] < 4 or x["off"] % 2) and has("P1", cap=8, path="four") and has("P1", cap=8, path="scalar")
    # P2
    assert all(x["path"] == "four" and x["off"] % 4 == 0 for x in pr["P2"])
    for cap in (4, 16, 64):
        for first in range(4):
            assert has("P2", cap=cap, first=first, found=True, steps=1) >= 1, (cap, first)
        assert sum(x["cap"] == cap and x["found"] and x["groups"] == 2 and not x["wrapped"] for x in pr["P2"]) >= (0 if cap == 4 else 2), cap
        assert has("P2", cap=cap, found=True, wrapped=True, groups=2) >= 2, cap
        assert sum(x["cap"] == cap and x["found"] and x["skipped_empty"] and x["steps"] >= 2 for x in pr["P2"]) >= 2, cap
        assert sum(x["cap"] == cap and not x["found"] and x["skipped_empty"] and x["groups"] == 2 for x in pr["P2"]) >= 1, cap
        assert has("P2", cap=cap, found=False, steps=2) >= 1, cap
    # P3
    assert all(x["path"] == "four" for x in pr["P3"])
    for cap in (16, 4):
        e_of = lambda x: (x["home"] - 1) % cap          # noqa: E731
        far = [x for x in pr["P3"] if x["cap"] == cap and x["found"] and x["steps"] == cap - 1]
        assert len(far) >= 60 and all(x["first"] == 1 and x["groups"] == cap // 4 and not x["round5"] and x["end"] == (e_of(x) - 1) % cap for x in far), cap
        assert cap == 4 or {e_of(x) for x in far} == {0, 4, 8, 12}
        for first in (1, 2, 3):
            out = [x for x in pr["P3"] if x["cap"] == cap and not x["found"] and x["first"] == first]
            assert len(out) >= 60 and all(x["round5"] and x["groups"] == cap // 4 + 1 and x["end"] % 4 == 0 and x["steps"] == cap - first + 1 for x in out), (cap, first)
        assert has("P3", cap=cap, found=False, steps=1) >= 60
    # P4
    c = C.case("P4")
    zero = {b: C.probe_census(c.T, b << 32) for b in (1, 8, 17, 5, 0)}
    assert (zero[1]["found"], zero[1]["steps"], zero[1]["pid"]) == (True, 1, 7) and (zero[8]["found"], zero[8]["steps"], zero[8]["pid"]) == (True, 2, 11)
    assert not zero[17]["found"] and zero[17]["steps"] == 1 and zero[17]["path"] == "four" and zero[17]["off"] % 4 == 2
    assert all(int(c.T.slots[zero[17]["off"] + s] >> np.uint64(32)) != C.EMPTY_VAL for s in (1, 15))
    assert not zero[5]["found"] and not zero[0]["found"] and zero[0]["cap"] == 1
    assert {zero[1]["path"], zero[8]["path"]} == {"scalar", "four"}
    low = np.bincount((c.kmers & np.uint64(0xffffffff)).astype(np.int64) % 1000003)                   # a low word held by four buckets
    shared = [int(k) for k in c.kmers if low[int(k & np.uint64(0xffffffff)) % 1000003] == 4 and int(k) & 0xffffffff]
    assert sorted(k >> 32 for k in shared) == [1, 5, 8, 17] and len({int(c.pids[np.searchsorted(c.kmers, np.uint64(k))]) for k in shared}) == 4
    assert has("P4", path="none") == 2
    for n in C.PROBE:                                           # the rows tell a hit's pattern apart: every probed word alone in the first buckets
        assert len(C.case(n).queries) >= 256 + 1 + 40


def test_walk_cases_hold_their_edges():
    """The walk census (Case.walk_census restates the visiting rule and the split of the sorted runs into workgroups of 512 / 1024).
    The LDS limits are what the engine's expression gives and what W4 uses.  W1: (workgroup, query) pairs that file 1023, 1024, 1025 and
    1500 long lists at either thread count, lists of 32 ids that file none, overflowing lists that end at N - 1.  W2: the hit patterns per
    query, 1 .. 300 k-mers per pattern; a workgroup boundary INSIDE a query where thread 0's climb ends at the previous hit's path; a last
    thread whose own node has hit descendants in the next workgroup; a node whose hit range starts in workgroup 0 and ends in workgroup 3
    (beyond the LDS stretch); a hit that is the ancestor of the next 600.  W3: P, the key widths, where the empty and all-miss queries
    stand, the repeated query, the last DFS node in the last query, a workgroup that spans more than 400 queries.  W5: the list lengths and run
    counts either side of 0xFFFF."""
    lim = C.lds_limits()
    assert lim == {512: 11008, 1024: 9984}, lim
    assert {C.case(n).N for n in C.LARGE[:4]} == {lim[512], lim[512] + 1, lim[1024], lim[1024] + 1}
    # W1
    c = C.case("W1")
    nloc = c.pat["num_local"].numpy()
    assert c.N == 128 and set(nloc[1:].tolist()) == {32, 33}
    for T in C.THREADS:
        runs, visited, groups = c.walk_census(T)
        for qi, target in enumerate(c.about["targets"]):
            mine = {k: v for k, v in groups.items() if k[1] == qi}
            if T == 1024 or qi < 4:
                assert len(mine) == 1 and list(mine.values())[0]["queued"] == target, (T, qi, mine)
            else:
                assert sum(v["queued"] for v in mine.values()) == target and len(mine) == 2
        assert sorted(v["queued"] for v in groups.values() if v["queued"] >= 1000)[:4] == [1023, 1024, 1025, 1500], T
        assert groups[max(k for k in groups if k[1] == 5)] == {"hits": 30, "queued": 0}                # the twins: lists of 32 ids
    d, pd, ld, se = c.layout()
    full = c.full()
    runs, visited, _ = c.walk_census(512)
    inv = np.argsort(d)
    over = [int(inv[r]) for (qi, _, _), v in zip(runs, visited) if qi in (2, 3) for r in v[:1]]         # (the first node of a late hit's climb)
    assert sum(int(c.pat["local_ids"][int(c.pat["local_ptr"][p + 1]) - 1]) == c.N - 1 for p in over) >= 100
    assert {n for _, _, n in runs} == {1, 2, 3} and all(f.size in (0, 32, 33, 64, 66, 96, 99) for f in full)
    # W2
    c = C.case("W2")
    d, pd, ld, se = c.layout()
    assert [c.hits(q)[0].size for q in c.queries] == [c.about["under"], 511, 512, 513, 1024, 1025] and c.about["under"] == 2016
    counts = np.concatenate([c.hits(q)[1] for q in c.queries])
    assert counts.min() == 1 and counts.max() == 300 and np.unique(counts).size >= 6
    for T in C.THREADS:
        runs, visited, groups = c.walk_census(T)
        inside = [i for i in range(T, len(runs), T) if runs[i][0] == runs[i - 1][0]]
        assert len(inside) >= 4 and all(pd[visited[i][-1]] >= 0 and pd[visited[i][-1]] <= runs[i - 1][1] for i in inside), T
        assert len({runs[i][0] for i in inside}) >= 3
        last = [i for i in range(T - 1, len(runs) - 1, T) if runs[i + 1][0] == runs[i][0] and se[runs[i][1]] > runs[i + 1][1]]
        assert last and visited[last[0]][0] == runs[last[0]][1], T
        if T == 512:
            assert [i for i in last if se[runs[i][1]] - runs[i][1] > 400] == [1023, 1535]
    runs, visited, groups = c.walk_census(512)
    R, A = int(d[c.about["R"]]), int(d[c.about["A"]])
    assert visited[0] == [A, R] and runs[0][:2] == (0, A) and se[R] - R == 2017 and se[A] - A == 601 and runs[600][1] == se[A] - 1
    assert sorted(k[0] for k in groups if k[1] == 0) == [0, 1, 2, 3]                                     # R's H: the hits of workgroups 0 .. 3
    assert int((ld > C.CK_IDS).sum()) >= 8
    # W3
    for name, P, pbits in (("W3a", 1023, 10), ("W3b", 1024, 11)):
        c = C.case(name)
        d, pd, ld, se = c.layout()
        nq = len(c.queries)
        assert c.P == P and C.key_bits(P, nq) == (pbits, 10) and nq == 613
        sizes = [q.size for q in c.queries]
        nhit = [c.hits(q)[0].size for q in c.queries]
        empty, miss = [i for i in range(nq) if not sizes[i]], [i for i in range(nq) if sizes[i] and not nhit[i]]
        assert len(empty) == len(miss) == 5 and empty[0] == 0 and miss[0] == 1 and empty[-1] == nq - 2 and miss[-1] == nq - 3
        assert 100 < empty[1] < 500 and 100 < miss[2] < 500
        assert sum(n == 1 for n in nhit) == 600 and sorted(set(nhit)) == [0, 1, nhit[300]] and nhit[300] >= 40
        rep = [i for i in range(nq) if nhit[i] > 1]
        assert len(rep) == 3 and rep[1] == rep[0] + 1 and rep[2] > rep[1] + 50 and all(np.array_equal(c.queries[i], c.queries[rep[0]]) for i in rep)
        runs, visited, groups = c.walk_census(512)
        assert runs[-1][:2] == (nq - 1, P - 1) and ((nq - 1) << pbits | (P - 1)) < (1 << (pbits + 10)) - 1
        assert any(h == 1 for _, h, _ in runs) and len({k[1] for k in groups if k[0] == 0}) >= 400 and len({k[1] for k in groups if k[0] == 1}) >= 150
        assert (d != np.arange(P)).any()
    # W4
    for n in C.LARGE[:4]:
        c = C.case(n)
        full, e = c.full(), c.about["edge"]
        nloc = c.pat["num_local"].numpy()
        lp, ids = c.pat["local_ptr"].numpy(), c.pat["local_ids"].numpy()
        ends = [int(ids[lp[p + 1] - 1]) for p in e if nloc[p] > C.CK_IDS]
        assert ends.count(c.N - 1) >= 3 and ends.count(c.N - 2) >= 3 and 2500 < c.P < 4000 and max(nloc) == 4000
        hit = set(np.concatenate([c.hits(q)[0] for q in c.queries]).tolist())
        assert set(e) <= hit and len(hit) > 800
    # W5
    c = C.case("W5")
    nloc = c.pat["num_local"].numpy()
    lp, ids = c.pat["local_ptr"].numpy(), c.pat["local_ids"].numpy()
    rts = c.about["roots"]
    assert c.N == 131200 and [int(nloc[r]) for r in rts] == [65534, 65535, 65536, 70000]
    n_runs = [1 + int((np.diff(ids[lp[r]: lp[r + 1]]) > 1).sum()) for r in rts]
    assert n_runs == [65534, 65535, 65536, 1] and -(-70000 // 4095) == 18          # (20 bits of start, 12 of length: a run of 70 000 ids is stored as 18)
    par = c.pat["parent"].numpy()
    assert all(par[par[g]] == r for g, r in zip(c.about["grand"], rts))
    assert [c.hits(q)[0].tolist() for q in c.queries[:4]] == [[g] for g in c.about["grand"]] and c.rows()[1, c.N - 1] == 3


# ------------------------------------------------------------------------------------------------------------------------------------
# on the device
# ------------------------------------------------------------------------------------------------------------------------------------
def _prefill(nq, N):
    """a fixed non-zero pattern, every seventh cell near 2^32 (the sums wrap there)"""
    i = np.arange(nq * N, dtype=np.uint64)
    pre = ((i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xffffffff)).astype(np.uint32)
    pre[::7] = np.uint32(0xffffffff) - (i[::7] % np.uint64(3)).astype(np.uint32)
    return pre.reshape(nq, N)


def _check_handle(K, d, c, exp, dev, tag, device_entry=True):
    import torch
    qs = c.queries
    _same(d.new2all(qs), exp, "%s: new2all" % (tag,))
    _same(d.new2all(qs), exp, "%s: second call" % (tag,))
    sp = d.new2all_sparse(qs)
    assert sp.n_rows == len(qs), tag
    for qi in range(len(qs)):
        col, val = sp.row(qi)
        nz = np.nonzero(exp[qi])[0]
        assert np.array_equal(col, nz) and np.array_equal(val, exp[qi][nz]), (tag, "sparse row", qi)
    if device_entry:
        pre = _prefill(len(qs), c.N)
        buf = torch.from_numpy(pre.view(np.int32).copy()).to(torch.device("cuda", dev))
        d.new2all_device(qs, buf.data_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint32)
        want = pre + exp                                        # uint32: wraps
        assert (want < pre).any() or not exp.any(), tag
        _same(got, want, "%s: new2all_device into a prefilled buffer" % (tag,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.NAMES)
def test_rows(K, dev, env, built, name):
    """new2all, a second call on the same handle, new2all_sparse (rows == the non-zeros) and new2all_device into a buffer prefilled with a
    fixed non-zero pattern (result == prefill + rows mod 2^32) == the definition, a fresh handle per environment of N2A_VARIANTS"""
    lap = _Lap("new2all conformance " + name)
    c = built(name)
    exp = c.rows()
    h = K.HostDB(c.path)
    lap("database, definition")
    for variant in N2A_VARIANTS:
        env(**variant)
        d = K.DeviceDB(h, device=dev, with_hashtables=True)
        try:
            _check_handle(K, d, c, exp, dev, (name, variant))
        finally:
            d.close()
        lap(",".join(variant) or "default")
    lap.done()


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.NAMES)
def test_query_shards(K, dev, env, built, name):
    """two and three query shards (tables repacked per shard in layout.hip: other offsets, other parities), their rows summed == the
    definition, under every environment of N2A_VARIANTS"""
    c = built(name)
    exp = c.rows()
    h = K.HostDB(c.path)
    for variant in N2A_VARIANTS:
        env(**variant)
        for shards in (2, 3):
            acc = np.zeros_like(exp)
            for s in range(shards):
                d = K.DeviceDB(h, device=dev, query_shard=(s, shards))
                try:
                    acc += d.new2all(c.queries)
                finally:
                    d.close()
            _same(acc, exp, "case %s, %d query shards, %s" % (name, shards, variant))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("W3a", "W3b"))
def test_batches_of_1_2_3_256_257_queries(K, dev, env, built, name):
    """slices of W3's batch as batches of their own: nq = 1 (an empty query; a hit), 2, 3, 256, 257, and the batch without its last one and
    two queries (it then ends with an empty / an all-miss query); default environment and KMDB_N2A_THREADS=1024"""
    c = built(name)
    exp = c.rows()
    h = K.HostDB(c.path)
    nq = len(c.queries)
    for variant in (N2A_VARIANTS[0], N2A_VARIANTS[3]):
        env(**variant)
        d = K.DeviceDB(h, device=dev, with_hashtables=True)
        try:
            for a, b in ((0, 1), (1, 2), (2, 3), (2, 4), (2, 5), (0, 3), (0, 256), (0, 257), (nq - 257, nq), (nq - 256, nq), (0, nq - 1), (0, nq - 2), (nq - 1, nq)):
                _same(d.new2all(c.queries[a:b]), exp[a:b], "case %s, queries [%d, %d), %s" % (name, a, b, variant))
        finally:
            d.close()


@pytest.mark.gpu
def test_queries_of_511_to_1025_hit_patterns_alone(K, dev, env, built):
    """every query of W2 as a batch of its own, once with its absent words and once without (no run of the all-ones key behind the hits:
    the batch's runs ARE its 511 / 512 / 513 / 1024 / 1025 / 2016 hit patterns, so a workgroup of 512 or 1024 threads ends exactly with
    the list, one short of it or one beyond — the entry beyond the workgroup is then csum[nruns], the end of the scan); default
    environment, 1024 threads, and KMDB_N2A_NO_RUNS + 1024 threads"""
    c = built("W2")
    exp = c.rows()
    hits_only = [q[np.isin(q, c.kmers)] for q in c.queries]
    assert [c.hits(q)[0].size for q in hits_only] == [2016, 511, 512, 513, 1024, 1025] and all(h.size < q.size for h, q in zip(hits_only[1:], c.queries[1:]))
    h = K.HostDB(c.path)
    for variant in (N2A_VARIANTS[0], N2A_VARIANTS[3], N2A_VARIANTS[4]):
        env(**variant)
        d = K.DeviceDB(h, device=dev, with_hashtables=True)
        try:
            for qi in range(len(c.queries)):
                _same(d.new2all([c.queries[qi]]), exp[qi: qi + 1], "case W2, query %d alone, %s" % (qi, variant))
                _same(d.new2all([hits_only[qi]]), exp[qi: qi + 1], "case W2, the hits of query %d alone, %s" % (qi, variant))
        finally:
            d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.PROBE)
def test_probe_tables_through_db2db(K, dev, built, tmp_path, name):
    """group P's tables under db2db's probe: the fabricated part as the row database, a second part that holds the probed words as the
    k-mers of 32 samples; the cell, both ways round, == the definition from the lists (gamma_cases.db2db_from_lists)"""
    import torch
    c = built(name)
    S = _S()
    pat, n, words, pids = C.probes_part(c)
    pat = dict(pat)
    pat["num_kmers"] = torch.from_numpy(np.bincount(pids, minlength=n + 1).astype(np.int64))
    path = str(tmp_path / "probes.db")
    S.write_db(path, C.K_LEN, 1.0, ["q%d" % i for i in range(n)], [1] * n, S.to_view_arrays(pat), kmers_count=int(words.size),
               tables=S.build_hashtables(torch.from_numpy(words.astype(np.int64)), torch.from_numpy(pids), C.K_LEN))
    _, ia, ib = np.intersect1d(c.kmers, words, assume_unique=True, return_indices=True)
    assert ia.size == c.kmers.size                               # every key of the fabricated tables is probed
    exp = db2db_from_lists(c.pat, c.N, c.pids[ia], pat, n, pids[ib])
    assert exp.any()
    a = K.DeviceDB(K.HostDB(c.path), device=dev, with_hashtables=True)
    b = K.DeviceDB(K.HostDB(path), device=dev, with_hashtables=True)
    try:
        _same(a.db2db(b), exp, "case %s, fabricated rows x probes" % name)
        _same(b.db2db(a), np.ascontiguousarray(exp.T), "case %s, probes x fabricated columns" % name)
    finally:
        a.close()
        b.close()
