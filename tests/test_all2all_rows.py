"""all2all -rows: a band of the matrix's rows computed on the device (kmdb_all2all_rows_device / kmdb_all2all_rows / kmdb_all2all_rows_stats_get,
KMDB_HAS_ALL2ALL_ROWS; the front-end's `all2all | all2all-sp -rows <lo>:<hi>`).  The definition: exactly the cells [tri(row_lo), tri(row_hi)) of
what kmdb_all2all_dense_device writes for the same handle.  The witness of every library test is the matrix from the definition in numpy over
the lists the test built (variant_cases.definition, or all2all_rows_cases.band_definition where the triangle is too large), and the stats of
every call are held against a host census (all2all_rows_cases.census): nodes_applied and updates are exact, nodes_selected is a superset."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import all2all_rows_cases as RC
import build_cases as BC
import extend_cases as EC
import minhash_cases as MC
import variant_cases as VC
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
HEADER = os.path.join(ROOT, "include", "kmdb_amd.h")
BUILD_DIR = os.path.join(ROOT, "kmer-db_amd", "build")
NEW_SYMBOLS = ("kmdb_all2all_rows_device", "kmdb_all2all_rows", "kmdb_all2all_rows_stats_get", "kmdb_device_buffer_alloc")
tri = RC.tri


def _cli(*args, cwd=None, ok=True, env=None):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, cwd=cwd, env=None if env is None else dict(os.environ, **env))
    if ok:
        assert r.returncode == 0, r.stderr
    return r


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_declared(K):
    src = EC.read(HEADER).decode()
    assert re.search(r"^#define KMDB_HAS_ALL2ALL_ROWS 1$", src, re.M)
    assert re.search(r"^#define KMDB_ABI_VERSION 8$", src, re.M)
    assert K.ABI_VERSION == 8 and K.lib().kmdb_abi_version() == 8
    L = ctypes.CDLL(K.lib_path())
    for name in NEW_SYMBOLS:
        assert name in K.capi.EXPORTS and hasattr(L, name), name
        assert re.search(r"^int\s+%s\(" % name, src, re.M), name
    assert "kmdb_device_buffer_free" in K.capi.EXPORTS and hasattr(L, "kmdb_device_buffer_free")
    m = re.search(r"typedef struct kmdb_all2all_rows_stats \{(.*?)\} kmdb_all2all_rows_stats;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decl = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|uint32_t|double)\s+([^;]+);", body) for n in names.split(",")]
    ctype = {"c_ulong": "uint64_t", "c_uint": "uint32_t", "c_double": "double"}
    assert decl == [(ctype[t.__name__], f) for f, t in K.capi._All2allRowsStats._fields_]
    assert "similarity_calculator.cpp:213-233" in src
    for meth in ("all2all_rows", "all2all_rows_device", "all2all_rows_stats"):
        assert hasattr(K.DeviceDB, meth), meth


def test_null_arguments_are_refused_by_name(K):
    lib = K.capi.lib()
    assert lib.kmdb_all2all_rows_device(None, 0, 0, None, None) != 0 and b"kmdb_all2all_rows_device: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows(None, 0, 0, None, None) != 0 and b"kmdb_all2all_rows: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows_stats_get(None, None) != 0 and b"kmdb_all2all_rows_stats_get: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_device_buffer_alloc(0, 16, None) != 0 and b"kmdb_device_buffer_alloc: null argument" in lib.kmdb_last_error()


def test_cli_refusals_by_name_and_usage(tmp_path):
    """refused before any file is read or any device touched: one ERROR line that names the switches, nothing written, the database (which does
    not exist) never mentioned"""
    db, out, old = str(tmp_path / "no_such.db"), str(tmp_path / "out.csv"), str(tmp_path / "no_such_old.db")
    for mode in ("all2all", "all2all-sp"):
        for args, words in (((mode, "-rows", "3:9", "-gpus", "2", db, out), ("-rows", "-gpus")),
                            ((mode, "-rows", "3:9", "-sample-rows", "jaccard:3", db, out), ("-rows", "-sample-rows")),
                            ((mode, "-rows", "3:9", "-phylip-out", "-distance", "mash", db, out), ("-rows", "-phylip-out")),
                            ((mode, "-rows", "new", db, out), ("-rows new", "-from-samples -extend-from")),
                            ((mode, "-from-samples", "-rows", "new", db, out), ("-rows new", "-from-samples -extend-from")),
                            ((mode, "-rows", "9:3", db, out), ("-rows", "lo > hi")),
                            ((mode, "-sparse", "-rows", "9:3", db, out), ("-rows", "lo > hi")),
                            ((mode, "-distance", "jaccard", "-rows", "9:3", db, out), ("-rows", "lo > hi")),
                            ((mode, "-rows", "3", db, out), ("-rows expects <lo>:<hi>",)),
                            ((mode, "-rows", "3:4:5", db, out), ("-rows expects <lo>:<hi>",)),
                            ((mode, "-rows", "a:7", db, out), ("-rows expects <lo>:<hi>",)),
                            ((mode, "-rows", "-1:7", db, out), ("-rows expects <lo>:<hi>",)),
                            ((mode, "-rows", "1:7x", db, out), ("-rows expects <lo>:<hi>",)),
                            ((mode, "-rows", "3:99999999999999999999", db, out), ("-rows expects <lo>:<hi>",))):
            r = _cli(*args, ok=False)
            assert r.returncode not in (0, -11, -6), (args, r.stderr)
            err = [ln for ln in r.stderr.splitlines() if ln.startswith("ERROR: ")]
            assert len(err) == 1 and all(w in err[0] for w in words), (args, r.stderr)
            assert "no_such" not in r.stderr and "Loading" not in r.stderr, (args, r.stderr)
            assert not os.path.exists(out), args
    for mode in ("new2all", "one2all", "all2all-parts", "build", "distance"):
        r = _cli(mode, "-rows", "3:9", db, out, ok=False)
        assert r.returncode != 0 and "-rows applies to all2all and all2all-sp" in r.stderr, (mode, r.stderr)
    # a well-formed band goes on to the file, which is not there
    r = _cli("all2all", "-rows", "3:", db, out, ok=False)
    assert r.returncode != 0 and "no_such.db" in r.stderr
    usage = _cli().stderr
    for line in ("    kmer-db-amd all2all | all2all-sp -rows <lo>:<hi> [the mode's own switches] <database> <output>",
                 "-rows new (with -from-samples -extend-from <old.db>): the rows of the samples added to <old.db>.",
                 "Refused with -gpus <N>, -sample-rows and -phylip-out, and when hi exceeds the sample count."):
        assert line in usage, line


def test_band_kernels_spill_nothing():
    """the compiler's resource remarks of a2a_rows.hip: both kernels without scratch and without a spilled register"""
    res = os.path.join(BUILD_DIR, "a2a_rows.resources.txt")
    if not os.path.isdir(BUILD_DIR):
        pytest.skip("the build directory %s is absent" % BUILD_DIR)
    assert os.path.exists(res), "%s is missing: the build writes it for every .hip source" % res
    found, cur = {}, None
    with open(res, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.match(r"_ZN12_GLOBAL__N_1\d+(rows_\w+_kernel)E", m.group(1))
                cur = found.setdefault(k.group(1), {}) if k else None
                continue
            m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
    assert set(found) == {"rows_select_kernel", "rows_apply_kernel"}
    for key, r in found.items():
        print(key, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (key, r)


def test_references_agree_on_small_forests():
    """the band reference and the census against the whole-matrix definition and a plain count (no device)"""
    for pat, N in (RC.tiny_forest(), RC.cut_forest(), RC.superset_forest(), RC.weight_forest(), RC.chain_forest(9, True)):
        full = VC.definition(pat, N)
        lists, w = VC.full_lists(pat), pat["num_kmers"].numpy()
        lp, ids, par = pat["local_ptr"].numpy(), pat["local_ids"].numpy(), pat["parent"].numpy()
        kids = [[c for c in range(len(par)) if par[c] == p] for p in range(len(par))]

        def subtree(p):
            return int(w[p]) + sum(subtree(c) for c in kids[p])
        for lo in range(N + 1):
            for hi in range(lo, N + 1):
                assert np.array_equal(RC.band_definition(pat, N, lo, hi), full[tri(lo): tri(hi)]), (lo, hi)
                applied = updates = 0
                for p, fl in enumerate(lists):
                    loc = ids[lp[p]: lp[p + 1]]
                    rows = [int(i) for i in loc if lo <= i < hi]
                    if loc.size and fl.size > 1 and subtree(p) % (1 << 32) and rows:
                        applied += 1
                        updates += sum(int(np.searchsorted(fl, i)) for i in rows)
                assert RC.census(pat, lo, hi) == (applied, updates), (lo, hi)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, library
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


@pytest.fixture(scope="module")
def S(K):
    return importlib.import_module("kmerdb_amd.synth")


@pytest.fixture(scope="module")
def virus(K, dev, golden_dir):
    """(HostDB with its tables, DeviceDB, the forest decoded from the file, the whole matrix) of virus_k18.db — computed once, never changed"""
    h = K.HostDB(os.path.join(golden_dir, "virus_k18.db"))
    d = K.DeviceDB(h, device=dev)
    full = d.all2all_dense()
    full.setflags(write=False)
    yield h, d, RC.pat_of_host(h), full
    d.close()


def _upload(K, S, pat, N, dev):
    _, view = VC.make_view(K, S, pat, N)
    return K.DeviceDB(view, device=dev)


def check_band(d, pat, N, lo, hi, exp):
    """one band call: the cells, and the stats against the census — the two equalities every test of this file asserts"""
    got = d.all2all_rows(lo, hi)
    assert got.dtype == np.uint32 and got.size == tri(hi) - tri(lo)
    assert np.array_equal(got, exp), "band [%d, %d): %d of %d cells differ" % (lo, hi, int((got != exp).sum()), exp.size)
    st = d.all2all_rows_stats()
    applied, updates = RC.census(pat, lo, hi)
    assert (st["nodes_applied"], st["updates"]) == (applied, updates), (lo, hi, st, applied, updates)
    assert st["nodes_selected"] >= st["nodes_applied"] and st["band_cells"] == exp.size, (lo, hi, st)
    st["cells"] = got
    return st


@pytest.mark.gpu
def test_every_band_of_a_tiny_forest(K, S, dev):
    pat, N = RC.tiny_forest()
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    assert np.array_equal(d.all2all_dense(), full)
    pairs = [(lo, hi) for lo in range(N + 1) for hi in range(lo, N + 1)]
    assert len(pairs) == 55
    for lo, hi in pairs:
        st = check_band(d, pat, N, lo, hi, full[tri(lo): tri(hi)])
        if lo == hi:
            assert st["nodes_selected"] == 0 and st["updates"] == 0
    st = check_band(d, pat, N, 0, N, full)
    assert st["scratch_bytes"] > 0 and st["select_ms"] > 0 and st["apply_ms"] > 0 and d.stats()["kernel_ms"] >= st["apply_ms"]
    d.close()


@pytest.mark.gpu
def test_band_ends_inside_a_local_list(K, S, dev):
    pat, N = RC.cut_forest()
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    for lo, hi in ((7, 12), (3, 4), (20, 21), (0, 3), (21, 21)):
        st = check_band(d, pat, N, lo, hi, full[tri(lo): tri(hi)])
        if (lo, hi) == (0, 3):
            assert st["nodes_selected"] == 1 and st["nodes_applied"] == 1            # the parent alone
        if (lo, hi) == (7, 12):
            assert st["nodes_selected"] == 1 and st["updates"] == 7 + 8 + 9 + 10 + 11
    d.close()


@pytest.mark.gpu
def test_the_superset_rule(K, S, dev):
    pat, N = RC.superset_forest()
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    st = check_band(d, pat, N, 10, 20, full[tri(10): tri(20)])
    assert st["nodes_selected"] == 2 and st["nodes_applied"] == 1 and st["updates"] == 1
    st = check_band(d, pat, N, 50, 51, full[tri(50): tri(51)])
    assert st["nodes_selected"] == st["nodes_applied"] == 1 and st["updates"] == 3
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("siblings", [False, True], ids=["chain", "siblings"])
@pytest.mark.parametrize("depth", [63, 64, 65, 130])
def test_ancestor_batches(K, S, dev, depth, siblings):
    pat, N = RC.chain_forest(depth, siblings)
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    check_band(d, pat, N, N - 2, N, full[tri(N - 2): tri(N)])
    check_band(d, pat, N, 0, N, full)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("l", [1024, 1025])
def test_long_lists(K, S, dev, l):
    """a list at and past the LDS stack (and DEC_CAP): the band strictly inside it, then across its end"""
    pat, N = RC.long_list_forest(l)
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    for lo, hi in ((500, 510), (N - 6, N), (0, 12)):
        check_band(d, pat, N, lo, hi, full[tri(lo): tri(hi)])
    d.close()


@pytest.mark.gpu
def test_a_list_past_any_lds_stack(K, S, dev):
    pat, N = RC.deep_forest()
    d = _upload(K, S, pat, N, dev)
    st = check_band(d, pat, N, 4090, 4100, RC.band_definition(pat, N, 4090, 4100))
    assert st["nodes_applied"] == 8 and st["scratch_bytes"] >= 4 * N
    d.close()


@pytest.mark.gpu
def test_64_bit_offsets_and_wide_codes(K, S, dev):
    """N = 70 002: the two rows are 560 KB where the triangle would be 9.8 GB; cell offsets beyond 2^31, a delta of 2^16 and more"""
    pat, N = RC.wide_code_forest()
    assert tri(70000) > (1 << 31)
    d = _upload(K, S, pat, N, dev)
    st = check_band(d, pat, N, 70000, 70002, RC.band_definition(pat, N, 70000, 70002))
    assert st["band_cells"] == 70000 + 70001 and st["nodes_applied"] == 6
    check_band(d, pat, N, 69999, 70000, RC.band_definition(pat, N, 69999, 70000))
    d.close()


@pytest.mark.gpu
def test_weights(K, S, dev):
    pat, N = RC.weight_forest()
    full = VC.definition(pat, N)
    assert int((VC.definition(pat, N, dtype=np.uint64) >= (1 << 32)).sum()) > 0
    d = _upload(K, S, pat, N, dev)
    assert np.array_equal(d.all2all_dense(), full)
    for lo, hi in ((0, N), (1, 4), (4, 8), (5, 6), (7, 8)):
        st = check_band(d, pat, N, lo, hi, full[tri(lo): tri(hi)])
    st = check_band(d, pat, N, 0, N, full)
    assert st["nodes_selected"] == 7              # of eleven: a subtree sum of 0 modulo 2^32, a subtree without weights and the empty pattern stay out
    d.close()


def _partition(d, pat, N, full, seeds=range(6)):
    for seed in seeds:
        cuts = RC.seeded_cuts(N, 1000 + seed, 2 + seed)
        parts = [check_band(d, pat, N, a, b, full[tri(a): tri(b)])["cells"] for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts), full), cuts


@pytest.mark.gpu
@pytest.mark.parametrize("N", [130, 257])
def test_partition_of_clade_collections(K, S, dev, N):
    g, pat = S.synth_database(N, 13, 1500, k=18, seed=7 + N, device="cpu")
    d = _upload(K, S, pat, N, dev)
    full = d.all2all_dense()
    assert np.array_equal(full, VC.definition(pat, N))
    _partition(d, pat, N, full)
    d.close()


@pytest.mark.gpu
def test_partition_of_the_virus_database(virus):
    h, d, pat, full = virus
    assert h.N == 165
    _partition(d, pat, h.N, full)


@pytest.mark.gpu
def test_partition_on_a_handed_over_builder(K, dev):
    """a handle from Builder.finish_device against the upload of the finished image"""
    names, lists = BC.shape_lists(BC.SHAPES[0])
    b1, b2 = K.Builder(BC.SHAPES[0][3], BC.SHAPES[0][4]), K.Builder(BC.SHAPES[0][3], BC.SHAPES[0][4])
    try:
        b1.add_kmers(names, lists)
        b2.add_kmers(names, lists)
        h1 = b1.finish()
        d1 = K.DeviceDB(h1, device=dev)
        d2, h2 = b2.finish_device()
    finally:
        b1.close()
        b2.close()
    full = d1.all2all_dense()
    _partition(d2, RC.pat_of_host(h1), d2.N, full)
    d1.close()
    d2.close()


def _band_tensor(d, lo, hi, dev):
    """the band in a torch tensor that held other values before (the buffer need not be zeroed)"""
    import torch
    t = torch.full((max(1, tri(hi) - tri(lo)),), -1, dtype=torch.int32, device=torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    d.all2all_rows_device(t.data_ptr(), lo, hi)
    return t


@pytest.mark.gpu
def test_consumers_sparse(K, dev, virus):
    h, d, pat, full = virus
    lo, hi = 100, 165
    t = _band_tensor(d, lo, hi, dev)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), full[tri(lo): tri(hi)])
    st = d.all2all_rows_stats()
    assert (st["nodes_applied"], st["updates"]) == RC.census(pat, lo, hi)
    for filters in ([], [("jaccard", 0.9, None)]):
        want = d.all2all_sparse_filtered(filters, h.sample_kmers)
        got = d.sparse_from_dense_device(t.data_ptr(), tri(lo), tri(hi), filters=filters, sample_kmers=h.sample_kmers)
        assert got.n_rows == h.N and int(got.row_ptr[lo]) == 0 and got.nnz == int(want.row_ptr[hi] - want.row_ptr[lo]) and got.nnz > 0
        for i in range(lo, hi):
            gc, gv = got.row(i)
            wc, wv = want.row(i)
            assert np.array_equal(gc, wc) and np.array_equal(gv, wv), i


@pytest.mark.gpu
@pytest.mark.parametrize("measure", ["jaccard", "mash"])
def test_consumers_distance(K, dev, virus, measure):
    h, d, pat, full = virus
    lo, hi = 100, 165
    whole = K.Distance(measure, h.k, h.sample_kmers, triangle=True, device=dev)
    whole.take_all2all(d, h.names)
    want = whole.matrix_rows(lo, hi)
    whole.close()
    t = _band_tensor(d, lo, hi, dev)
    st = d.all2all_rows_stats()
    assert (st["nodes_applied"], st["updates"]) == RC.census(pat, lo, hi)
    band = K.Distance(measure, h.k, h.sample_kmers, triangle=True, device=dev)
    band.take_cells(t.data_ptr(), lo, h.names)
    got = band.matrix_rows(lo, hi)
    band.close()
    assert len(want) > 1000 and got == want


@pytest.mark.gpu
def test_refusals(K, S, dev, golden_dir, virus):
    h, d, pat, full = virus
    N = h.N
    lib = K.capi.lib()
    o = K.capi._opts(dev)
    assert lib.kmdb_all2all_rows_device(d._d, 3, 9, None, ctypes.byref(o)) != 0 and b"kmdb_all2all_rows_device: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows(d._d, 3, 9, None, ctypes.byref(o)) != 0 and b"kmdb_all2all_rows: null argument" in lib.kmdb_last_error()
    t = _band_tensor(d, 0, 2, dev)
    for call, who in ((lambda *a, **kw: d.all2all_rows(*a, **kw), "kmdb_all2all_rows"),
                      (lambda *a, **kw: d.all2all_rows_device(t.data_ptr(), *a, **kw), "kmdb_all2all_rows_device")):
        with pytest.raises(K.KmdbError, match=who + r": row_lo > row_hi \(9 > 3\)"):
            call(9, 3)
        with pytest.raises(K.KmdbError, match=who + ": row_hi 166 > the 165 samples"):
            call(3, N + 1)
        with pytest.raises(K.KmdbError, match=who + r": a band needs the whole pattern stream \(shard_count must be 1\)"):
            call(3, 9, shard=(0, 2))
        with pytest.raises(K.KmdbError, match=who + ": unknown bits in kmdb_opts.flags"):
            call(3, 9, flags=1 << 9)
    # a call after a refusal still works, an empty band succeeds
    check_band(d, pat, N, 3, 9, full[tri(3): tri(9)])
    for lo, hi in ((7, 7), (0, 0), (0, 1), (N, N)):
        assert d.all2all_rows(lo, hi).size == 0
        d.all2all_rows_device(None, lo, hi)
        assert d.all2all_rows_stats()["band_cells"] == 0
    # a query shard
    q = K.DeviceDB(h, device=dev, query_shard=(0, 2))
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows: not on a query shard"):
        q.all2all_rows(3, 9)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_device: not on a query shard"):
        q.all2all_rows_device(t.data_ptr(), 3, 9)
    q.close()
    # a prefix shard is a handle like any other: its partial band
    p = K.DeviceDB(h, device=dev, prefix_shard=(1, 3))
    assert np.array_equal(p.all2all_rows(100, 165), p.all2all_dense()[tri(100): tri(165)])
    p.close()
    check_band(d, pat, N, 100, 165, full[tri(100): tri(165)])


@pytest.mark.gpu
def test_a_band_beyond_the_device_is_refused(K, S, dev):
    """N = 500 000: all rows are 2^32 cells and more and half a terabyte — refused with the bytes; the last row alone (its first cell lies
    beyond 2^36) is computed"""
    pat, N = RC.huge_forest()
    d = _upload(K, S, pat, N, dev)
    t = _band_tensor(d, 0, 2, dev)
    with pytest.raises(K.KmdbError, match=r"kmdb_all2all_rows_device: the band is 124999750000 cells, 499999000000 bytes, beyond the \d+ bytes of device memory"):
        d.all2all_rows_device(t.data_ptr(), 0, N)
    lib = K.capi.lib()
    o = K.capi._opts(dev)
    one = np.zeros(1, np.uint32)
    assert lib.kmdb_all2all_rows(d._d, 0, N, one.ctypes.data, ctypes.byref(o)) != 0
    assert re.search(rb"kmdb_all2all_rows: the band is 124999750000 cells, 499999000000 bytes, beyond the \d+ bytes of free device memory", lib.kmdb_last_error())
    st = check_band(d, pat, N, N - 1, N, RC.band_definition(pat, N, N - 1, N))
    assert st["updates"] == 3 + 1 and tri(N - 1) > (1 << 36)
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, front-end: the header lines of the full run's output, then exactly its lines of samples lo .. hi - 1
# ------------------------------------------------------------------------------------------------------------------------------------
def _lines(path):
    return EC.read(path).splitlines(keepends=True)


@pytest.fixture()
def fe(dev, golden_dir, tmp_path):
    return (lambda n: os.path.join(golden_dir, n)), (lambda n: str(tmp_path / n))


@pytest.mark.gpu
def test_front_end_dense(fe):
    g, t = fe
    want = _lines(g("virus.k18.csv"))
    assert len(want) == 167
    r = _cli("all2all", "-rows", "100:", g("virus_k18.db"), t("a.csv"), env={"KMDB_VERBOSE": "1"})
    assert _lines(t("a.csv")) == want[:2] + want[102:167]
    m = re.search(r"\[kmdb\] all2all rows: (\d+) cells, nodes selected / applied / updates (\d+) / (\d+) / (\d+), select \S+ ms, apply \S+ ms", r.stderr)
    assert m and int(m.group(1)) == tri(165) - tri(100) and int(m.group(2)) >= int(m.group(3)) > 0, r.stderr
    _cli("all2all", "-rows", "0:165", g("virus_k18.db"), t("b.csv"))
    assert EC.read(t("b.csv")) == EC.read(g("virus.k18.csv"))
    _cli("all2all", "-rows", ":", g("virus_k18.db"), t("b2.csv"))
    assert EC.read(t("b2.csv")) == EC.read(g("virus.k18.csv"))
    _cli("all2all", "-rows", "7:7", g("virus_k18.db"), t("c.csv"))
    assert _lines(t("c.csv")) == want[:2]
    _cli("all2all", "-rows", ":3", g("virus_k18.db"), t("d.csv"))
    assert _lines(t("d.csv")) == want[:5]
    for band in ("100:166", "166:", "166:166"):
        r = _cli("all2all", "-rows", band, g("virus_k18.db"), t("e.csv"), ok=False)
        err = [ln for ln in r.stderr.splitlines() if ln.startswith("ERROR: ")]
        assert r.returncode not in (0, -11, -6) and len(err) == 1 and "-rows" in err[0] and "165 samples" in err[0], (band, r.stderr)


@pytest.mark.gpu
def test_front_end_sparse(fe):
    g, t = fe
    want = _lines(g("virus.k18.sparse.csv"))
    assert len(want) == 167
    _cli("all2all", "-sparse", "-rows", "100:", g("virus_k18.db"), t("a.csv"))
    assert _lines(t("a.csv")) == want[:2] + want[102:167]
    _cli("all2all-sp", "-rows", "100:", g("virus_k18.db"), t("b.csv"))
    assert _lines(t("b.csv")) == want[:2] + want[102:167]
    _cli("all2all-sp", "-rows", "0:165", g("virus_k18.db"), t("c.csv"))
    assert EC.read(t("c.csv")) == EC.read(g("virus.k18.sparse.csv"))
    _cli("all2all-sp", "-rows", "7:7", g("virus_k18.db"), t("d.csv"))
    assert _lines(t("d.csv")) == want[:2]
    # the -min / -max list: against the full run with the same list
    sw = ("-min", "jaccard:0.5", "-max", "num-kmers:20000")
    _cli("all2all-sp", *sw, g("virus_k18.db"), t("f.want"))
    full = _lines(t("f.want"))
    _cli("all2all-sp", *sw, "-rows", "40:120", g("virus_k18.db"), t("f.csv"))
    assert _lines(t("f.csv")) == full[:2] + full[42:122] and len(EC.read(t("f.csv"))) < len(EC.read(t("c.csv")))
    _cli("all2all", "-sparse", *sw, "-rows", "40:120", g("virus_k18.db"), t("f2.csv"))
    assert EC.read(t("f2.csv")) == EC.read(t("f.csv"))


@pytest.mark.gpu
def test_front_end_distance(fe):
    g, t = fe
    want = _lines(g("virus.k18.csv.jaccard"))
    assert len(want) == 166
    _cli("all2all", "-distance", "jaccard", "-rows", "100:", g("virus_k18.db"), t("j.csv"))
    assert _lines(t("j.csv")) == want[:1] + want[101:166]
    # two measures from one band, the sparse form with a bound: against the full run
    sw = ("-distance", "ani", "-distance", "min", "-min", "0.5")
    _cli("all2all-sp", *sw, g("virus_k18.db"), t("two.want"))
    _cli("all2all-sp", *sw, "-rows", "30:101", g("virus_k18.db"), t("two.got"), env={"KMDB_DISTANCE_CELLS_PER_PIECE": "150"})
    for suffix in (".ani", ".min"):
        full = _lines(t("two.want" + suffix))
        assert len(full) == 166 and _lines(t("two.got" + suffix)) == full[:1] + full[31:102], suffix


@pytest.mark.gpu
def test_front_end_rows_new(fe, golden_dir, tmp_path):
    """the reference's extend workflow in one command: part 1 from its stored database, part 2 from its genomes, the rows of part 2 alone"""
    g, t = fe
    root = MC.link_virus_data(golden_dir, str(tmp_path))
    want = _lines(g("virus.k18.csv"))
    r = _cli("all2all", "-from-samples", "-extend-from", g("virus_k18_part1.db"), "-rows", "new", g("virus.seqs.part2.list"), t("new.csv"), cwd=root)
    assert "Calculating" in r.stderr
    assert _lines(t("new.csv")) == want[:2] + want[-65:]
    sp = _lines(g("virus.k18.sparse.csv"))
    _cli("all2all-sp", "-from-samples", "-extend-from", g("virus_k18_part1.db"), "-rows", "new", g("virus.seqs.part2.list"), t("new.sp.csv"), cwd=root)
    assert _lines(t("new.sp.csv")) == sp[:2] + sp[-65:]
