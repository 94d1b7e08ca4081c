"""all2all -band-rows: the band of the matrix with its rows summed in LDS tiles (kmdb_all2all_rows_tiled_device / kmdb_all2all_rows_tiled /
kmdb_all2all_rows_tiled_stats_get, KMDB_HAS_ALL2ALL_ROWS_TILED), a sparse run walked in such bands (kmdb_all2all_sparse_filtered_banded /
kmdb_all2all_banded_stats_get) and the front-end's `all2all | all2all-sp -band-rows <R>`.  The definition of the tiled call: bit for bit what
kmdb_all2all_rows_device writes for the same arguments.  Every library check holds the cells against the definition in numpy AND against the
existing band call, nodes_applied and updates against all2all_rows_cases.census, hits and jobs against the censuses of
all2all_rows_tiled_cases, and asserts runs <= updates and nodes_selected >= nodes_applied."""
import contextlib
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import all2all_rows_cases as RC
import all2all_rows_tiled_cases as TC
import extend_cases as EC
import minhash_cases as MC
import variant_cases as VC
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
HEADER = os.path.join(ROOT, "include", "kmdb_amd.h")
BUILD_DIR = os.path.join(ROOT, "kmer-db_amd", "build")
NEW_SYMBOLS = ("kmdb_all2all_rows_tiled_device", "kmdb_all2all_rows_tiled", "kmdb_all2all_rows_tiled_stats_get", "kmdb_all2all_sparse_filtered_banded",
               "kmdb_all2all_banded_stats_get")
tri = RC.tri


def _cli(*args, cwd=None, ok=True, env=None):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, cwd=cwd, env=None if env is None else dict(os.environ, **env))
    if ok:
        assert r.returncode == 0, r.stderr
    return r


@contextlib.contextmanager
def switches(tile_cols=None, tile_hits=None):
    """KMDB_ROWS_TILE_COLS / KMDB_ROWS_TILE_HITS for the calls inside (the library reads them at every call)"""
    want = {"KMDB_ROWS_TILE_COLS": tile_cols, "KMDB_ROWS_TILE_HITS": tile_hits}
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_declared(K):
    src = EC.read(HEADER).decode()
    assert re.search(r"^#define KMDB_HAS_ALL2ALL_ROWS_TILED 1$", src, re.M)
    assert re.search(r"^#define KMDB_ABI_VERSION 8$", src, re.M)
    L = ctypes.CDLL(K.lib_path())
    for name in NEW_SYMBOLS:
        assert name in K.capi.EXPORTS and hasattr(L, name), name
        assert re.search(r"^int\s+%s\(" % name, src, re.M), name
    ctype = {"c_ulong": "uint64_t", "c_uint": "uint32_t", "c_double": "double"}
    for struct, fields in (("kmdb_all2all_rows_tiled_stats", K.capi._All2allRowsTiledStats._fields_), ("kmdb_all2all_banded_stats", K.capi._All2allBandedStats._fields_)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        decl = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|uint32_t|double)\s+([^;]+);", body) for n in names.split(",")]
        assert decl == [(ctype[t.__name__], f) for f, t in fields], struct
    assert [f for f, _ in K.capi._All2allRowsTiledStats._fields_] == ["nodes_selected", "nodes_applied", "hits", "jobs", "runs", "updates", "tile_cols", "band_cells",
                                                                      "select_ms", "hits_ms", "apply_ms", "scratch_bytes"]
    for meth in ("all2all_rows_tiled", "all2all_rows_tiled_device", "all2all_rows_tiled_stats", "all2all_sparse_filtered_banded", "all2all_banded_stats"):
        assert hasattr(K.DeviceDB, meth), meth


def test_null_arguments_are_refused_by_name(K):
    lib = K.capi.lib()
    assert lib.kmdb_all2all_rows_tiled_device(None, 0, 0, None, None) != 0 and b"kmdb_all2all_rows_tiled_device: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows_tiled(None, 0, 0, None, None) != 0 and b"kmdb_all2all_rows_tiled: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows_tiled_stats_get(None, None) != 0 and b"kmdb_all2all_rows_tiled_stats_get: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_sparse_filtered_banded(None, 5, None, 0, None, -1, None, None) != 0
    assert b"kmdb_all2all_sparse_filtered_banded: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_banded_stats_get(None, None) != 0 and b"kmdb_all2all_banded_stats_get: null argument" in lib.kmdb_last_error()


def test_cli_refusals_by_name_and_usage(tmp_path):
    """refused before any file is read or any device touched: one ERROR line that names the switches, nothing written, the database (which does
    not exist) never mentioned"""
    db, out = str(tmp_path / "no_such.db"), str(tmp_path / "out.csv")
    for mode in ("all2all", "all2all-sp"):
        for args, words in (((mode, "-band-rows", "40", "-gpus", "2", db, out), ("-band-rows", "-gpus")),
                            ((mode, "-band-rows", "40", "-sample-rows", "jaccard:3", db, out), ("-band-rows", "-sample-rows")),
                            ((mode, "-band-rows", "40", "-phylip-out", "-distance", "mash", db, out), ("-band-rows", "-phylip-out")),
                            ((mode, "-band-rows", "0", db, out), ("-band-rows expects <R>",)),
                            ((mode, "-sparse", "-band-rows", "0", db, out), ("-band-rows expects <R>",)),
                            ((mode, "-distance", "jaccard", "-band-rows", "000", db, out), ("-band-rows expects <R>",)),
                            ((mode, "-band-rows", "4x", db, out), ("-band-rows expects <R>",)),
                            ((mode, "-band-rows", "-3", db, out), ("-band-rows expects <R>",)),
                            ((mode, "-band-rows", "3:9", db, out), ("-band-rows expects <R>",)),
                            ((mode, "-band-rows", "99999999999999999999", db, out), ("-band-rows expects <R>",)),
                            ((mode, db, out, "-band-rows"), ("-band-rows expects <R>",))):
            r = _cli(*args, ok=False)
            assert r.returncode not in (0, -11, -6), (args, r.stderr)
            err = [ln for ln in r.stderr.splitlines() if ln.startswith("ERROR: ")]
            assert len(err) == 1 and all(w in err[0] for w in words), (args, r.stderr)
            assert "no_such" not in r.stderr and "Loading" not in r.stderr, (args, r.stderr)
            assert not os.path.exists(out), args
    for mode in ("new2all", "one2all", "all2all-parts", "build", "distance", "minhash"):
        r = _cli(mode, "-band-rows", "40", db, out, ok=False)
        assert r.returncode != 0 and "-band-rows applies to all2all and all2all-sp" in r.stderr and "no_such" not in r.stderr, (mode, r.stderr)
    # a well-formed run goes on to the file, which is not there
    r = _cli("all2all", "-band-rows", "40", db, out, ok=False)
    assert r.returncode != 0 and "no_such.db" in r.stderr
    usage = _cli().stderr
    for line in ("    kmer-db-amd all2all | all2all-sp -band-rows <R> [the mode's own switches] <database> <output>",
                 "all2all / all2all-sp -band-rows <R>: the whole run walked in bands of R rows",
                 "KMDB_ROWS_TILED=1: plain -rows takes the tiled call too."):
        assert line in usage, line
    assert "Not offered: a whole run walked in bands" not in usage and "(-band-rows)" not in usage


FORESTS = {"tiny": RC.tiny_forest, "cut": RC.cut_forest, "weight": RC.weight_forest}


@pytest.mark.parametrize("name", sorted(FORESTS))
@pytest.mark.parametrize("tile_cols", [64, 4])
def test_the_run_form_is_the_definition(name, tile_cols):
    """difference entries per tile and a uint32 prefix sum give the band of the definition, for every band of the small forests; the additions
    the runs stand for are the census's"""
    pat, N = FORESTS[name]()
    for lo in range(N + 1):
        for hi in range(lo, N + 1):
            cells, runs, updates = TC.band_by_runs(pat, N, lo, hi, tile_cols)
            assert np.array_equal(cells, RC.band_definition(pat, N, lo, hi)), (lo, hi)
            assert updates == RC.census(pat, lo, hi)[1] and runs <= updates, (lo, hi)


def test_the_run_form_at_the_tile_edges():
    pat, N = TC.tile_edge_forest()
    cells, runs, updates = TC.band_by_runs(pat, N, 0, N, 64)
    assert np.array_equal(cells, VC.definition(pat, N)) and updates == RC.census(pat, 0, N)[1] and runs * 8 <= updates


def test_censuses_against_brute_force():
    for pat, N in (RC.tiny_forest(), RC.cut_forest(), RC.superset_forest(), RC.weight_forest(), RC.chain_forest(9, True), TC.five_hits_forest(),
                   TC.tile_edge_forest()):
        lists, w = VC.full_lists(pat), pat["num_kmers"].numpy()
        lp, ids, par = pat["local_ptr"].numpy(), pat["local_ids"].numpy(), pat["parent"].numpy()
        kids = [[c for c in range(len(par)) if par[c] == p] for p in range(len(par))]

        def subtree(p):
            return int(w[p]) + sum(subtree(c) for c in kids[p])
        good = [ids[lp[p]: lp[p + 1]].size and lists[p].size > 1 and subtree(p) % (1 << 32) for p in range(len(par))]
        bands = [(lo, hi) for lo in range(N + 1) for hi in range(lo, N + 1)] if N < 30 else [(0, N), (64, 66), (N - 5, N), (69, 70), (10, 10)]
        for lo, hi in bands:
            per_row = {}
            for p in range(len(par)):
                if good[p]:
                    for i in ids[lp[p]: lp[p + 1]]:
                        if lo <= i < hi:
                            per_row[int(i)] = per_row.get(int(i), 0) + 1
            assert TC.hits(pat, lo, hi) == sum(per_row.values()), (lo, hi)
            assert len({p for _, p in TC.hit_list(pat, lo, hi)}) == RC.census(pat, lo, hi)[0]
            for T, H in ((64, 1), (4, 2), (16384, 256), (64, 3)):
                want = 0
                for r, h in per_row.items():
                    tiles = len(range(0, r, T))
                    shares = len(range(0, h, H))
                    want += tiles * shares
                assert TC.jobs(pat, lo, hi, T, H) == want, (lo, hi, T, H)


def test_band_kernels_spill_nothing():
    """the compiler's resource remarks of a2a_band.hip: every kernel of the file without scratch and without a spilled register"""
    res = os.path.join(BUILD_DIR, "a2a_band.resources.txt")
    if not os.path.isdir(BUILD_DIR):
        pytest.skip("the build directory %s is absent" % BUILD_DIR)
    assert os.path.exists(res), "%s is missing: the build writes it for every .hip source" % res
    found, cur = {}, None
    with open(res, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.match(r"_ZN12_GLOBAL__N_1\d+(band_\w+_kernel)", m.group(1))
                cur = found.setdefault(m.group(1), {}) if k else None
                if k:
                    cur["kernel"] = k.group(1)
                continue
            m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
    assert {r["kernel"] for r in found.values()} == {"band_select_kernel", "band_hits_kernel", "band_apply_kernel"} and len(found) == 4     # (hits: count and write)
    for key, r in found.items():
        print(key, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (key, r)


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
    """(HostDB, DeviceDB, the forest decoded from the file, the whole matrix) of virus_k18.db — computed once, never changed"""
    h = K.HostDB(os.path.join(golden_dir, "virus_k18.db"))
    d = K.DeviceDB(h, device=dev)
    full = d.all2all_dense()
    full.setflags(write=False)
    yield h, d, RC.pat_of_host(h), full
    d.close()


def _upload(K, S, pat, N, dev):
    _, view = VC.make_view(K, S, pat, N)
    return K.DeviceDB(view, device=dev)


def check_tiled(d, pat, N, lo, hi, exp, tile_cols=None, tile_hits=None):
    """one tiled band call under the switches given: the cells against the definition and the existing band call, every stat against its census"""
    with switches(tile_cols, tile_hits):
        got = d.all2all_rows_tiled(lo, hi)
        st = d.all2all_rows_tiled_stats()
    assert got.dtype == np.uint32 and got.size == tri(hi) - tri(lo)
    assert np.array_equal(got, exp), "band [%d, %d): %d of %d cells differ from the definition" % (lo, hi, int((got != exp).sum()), exp.size)
    assert np.array_equal(got, d.all2all_rows(lo, hi)), "band [%d, %d) differs from kmdb_all2all_rows" % (lo, hi)
    T, H = tile_cols or TC.DEFAULT_TILE_COLS, tile_hits or TC.DEFAULT_TILE_HITS
    applied, updates = RC.census(pat, lo, hi)
    print("band [%d, %d) T %d H %d: %s" % (lo, hi, T, H, st))
    assert (st["nodes_applied"], st["updates"]) == (applied, updates), (lo, hi, st, applied, updates)
    assert (st["hits"], st["jobs"]) == (TC.hits(pat, lo, hi), TC.jobs(pat, lo, hi, T, H)), (lo, hi, st)
    assert st["runs"] <= st["updates"] and st["nodes_selected"] >= st["nodes_applied"], (lo, hi, st)
    assert st["band_cells"] == exp.size and st["tile_cols"] == T, (lo, hi, st)
    st["cells"] = got
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("sw", [(None, None), (64, 1)], ids=["default", "cols64-hits1"])
def test_every_band_of_a_tiny_forest(K, S, dev, sw):
    pat, N = RC.tiny_forest()
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    pairs = [(lo, hi) for lo in range(N + 1) for hi in range(lo, N + 1)]
    assert len(pairs) == 55
    for lo, hi in pairs:
        st = check_tiled(d, pat, N, lo, hi, full[tri(lo): tri(hi)], *sw)
        if lo == hi:
            assert st["nodes_selected"] == 0 and st["updates"] == 0 and st["jobs"] == 0
    st = check_tiled(d, pat, N, 0, N, full, *sw)
    assert st["scratch_bytes"] > 0 and st["select_ms"] > 0 and st["hits_ms"] > 0 and st["apply_ms"] > 0 and d.stats()["kernel_ms"] >= st["apply_ms"]
    d.close()


@pytest.mark.gpu
def test_band_edges(K, S, dev):
    """a run clipped at the row's own id; a node selected without a hit"""
    pat, N = RC.cut_forest()
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    for lo, hi in ((7, 12), (3, 4), (20, 21), (0, 3), (21, 21)):
        st = check_tiled(d, pat, N, lo, hi, full[tri(lo): tri(hi)])
        if (lo, hi) == (7, 12):
            assert st["nodes_selected"] == 1 and st["hits"] == 5 and st["updates"] == 7 + 8 + 9 + 10 + 11 and st["runs"] == 2 * 5
    d.close()
    pat, N = RC.superset_forest()
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    st = check_tiled(d, pat, N, 10, 20, full[tri(10): tri(20)])
    assert st["nodes_selected"] == 2 and st["nodes_applied"] == 1 and st["hits"] == 1 and st["updates"] == 1
    st = check_tiled(d, pat, N, 50, 51, full[tri(50): tri(51)])
    assert st["nodes_selected"] == st["nodes_applied"] == 1 and st["updates"] == 3
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("siblings", [False, True], ids=["chain", "siblings"])
@pytest.mark.parametrize("depth", [63, 64, 65, 130])
def test_chain_batches(K, S, dev, depth, siblings):
    """root paths of 63 / 64 / 65 / 130 nodes: the 64-lane chain batches; with siblings several hits on one row"""
    pat, N = RC.chain_forest(depth, siblings)
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    check_tiled(d, pat, N, N - 2, N, full[tri(N - 2): tri(N)])
    check_tiled(d, pat, N, 0, N, full)
    check_tiled(d, pat, N, 0, N, full, 64, 2)
    d.close()


@pytest.mark.gpu
def test_tile_edges(K, S, dev):
    pat, N = TC.tile_edge_forest()
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    for lo, hi in ((64, 66), (128, 130), (300, 304), (63, 65), (199, 200)):
        st = check_tiled(d, pat, N, lo, hi, full[tri(lo): tri(hi)], 64)
        if (lo, hi) == (64, 66):
            # the root's rows 64 (one tile) and 65 (a tile of 64 columns and one of 1); {64 .. 80, 301} is a hit of both and holds column 64 of row 65
            assert st["hits"] == 4 and st["jobs"] == 1 + 2 and st["runs"] == 1 + 2 + 1 and st["updates"] == 64 + 65 + 1
        if (lo, hi) == (128, 130):
            assert st["jobs"] == 2 + 3 and st["runs"] == 5
    st = check_tiled(d, pat, N, 0, N, full, 64)
    assert st["runs"] * 8 <= st["updates"], st
    assert st["runs"] == TC.band_by_runs(pat, N, 0, N, 64)[1]
    check_tiled(d, pat, N, 0, N, full, 64, 1)
    check_tiled(d, pat, N, 0, N, full, 128)
    check_tiled(d, pat, N, 0, N, full)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tile_hits", [1, 2, 3])
def test_shares(K, S, dev, tile_hits):
    pat, N = TC.five_hits_forest()
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    assert TC.hits(pat, 69, 70) == 5
    st = check_tiled(d, pat, N, 69, 70, full[tri(69): tri(70)], None, tile_hits)
    assert st["jobs"] == -(-5 // tile_hits)
    st = check_tiled(d, pat, N, 69, 70, full[tri(69): tri(70)], 64, tile_hits)
    assert st["jobs"] == 2 * -(-5 // tile_hits)
    check_tiled(d, pat, N, 0, N, full, 64, tile_hits)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("l", [1024, 1025])
def test_long_lists(K, S, dev, l):
    pat, N = RC.long_list_forest(l)
    full = VC.definition(pat, N)
    d = _upload(K, S, pat, N, dev)
    for lo, hi in ((500, 510), (N - 6, N), (0, 12)):
        check_tiled(d, pat, N, lo, hi, full[tri(lo): tri(hi)])
    check_tiled(d, pat, N, 500, 510, full[tri(500): tri(510)], 64, 1)
    # more than 1024 rows: the hit passes go to the rows' counters directly; 1024 and fewer: through the workgroup's LDS counts
    assert N > 1024 + 5
    check_tiled(d, pat, N, 0, N, full)
    check_tiled(d, pat, N, 5, 1029, full[tri(5): tri(1029)])
    check_tiled(d, pat, N, 5, 1030, full[tri(5): tri(1030)])
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tile_cols", [None, 1024])
def test_a_deep_chain(K, S, dev, tile_cols):
    pat, N = RC.deep_forest()
    d = _upload(K, S, pat, N, dev)
    st = check_tiled(d, pat, N, 4090, 4100, RC.band_definition(pat, N, 4090, 4100), tile_cols)
    assert st["nodes_applied"] == 8 and st["hits"] == 10
    d.close()


@pytest.mark.gpu
def test_64_bit_offsets_and_wide_codes(K, S, dev):
    """N = 70 002: cell offsets beyond 2^31, a delta of 2^16 and more, rows of several tiles"""
    pat, N = RC.wide_code_forest()
    assert tri(70000) > (1 << 31)
    d = _upload(K, S, pat, N, dev)
    st = check_tiled(d, pat, N, 70000, 70002, RC.band_definition(pat, N, 70000, 70002))
    assert st["band_cells"] == 70000 + 70001 and st["nodes_applied"] == 6
    assert st["jobs"] == 2 * len(range(0, 70000, TC.DEFAULT_TILE_COLS)) == 2 * 5 and st["hits"] > 2      # five tiles a row, one share of the row's hits each
    check_tiled(d, pat, N, 69999, 70000, RC.band_definition(pat, N, 69999, 70000), TC.MAX_TILE_COLS)
    d.close()


@pytest.mark.gpu
def test_weights(K, S, dev):
    """subtree sums that wrap: -W modulo 2^32 in the closing entries, a subtree sum of exactly 0"""
    pat, N = RC.weight_forest()
    full = VC.definition(pat, N)
    assert int((VC.definition(pat, N, dtype=np.uint64) >= (1 << 32)).sum()) > 0
    d = _upload(K, S, pat, N, dev)
    for lo in range(N + 1):
        for hi in range(lo, N + 1):
            check_tiled(d, pat, N, lo, hi, full[tri(lo): tri(hi)])
    st = check_tiled(d, pat, N, 0, N, full, 64, 1)
    assert st["nodes_selected"] == 7
    d.close()


def _partition(d, pat, N, full, seeds=range(6)):
    for seed in seeds:
        cuts = RC.seeded_cuts(N, 1000 + seed, 2 + seed)
        parts = [check_tiled(d, pat, N, a, b, full[tri(a): tri(b)])["cells"] for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts), full), cuts


@pytest.mark.gpu
@pytest.mark.parametrize("N", [130, 257])
def test_partition_of_clade_collections(K, S, dev, N):
    g, pat = S.synth_database(N, 13, 1500, k=18, seed=7 + N, device="cpu")
    d = _upload(K, S, pat, N, dev)
    full = d.all2all_dense()
    assert np.array_equal(full, VC.definition(pat, N))
    _partition(d, pat, N, full, seeds=range(3))
    cuts = RC.seeded_cuts(N, 77, 4)
    parts = [check_tiled(d, pat, N, a, b, full[tri(a): tri(b)], 64, 3)["cells"] for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate(parts), full)
    d.close()


@pytest.mark.gpu
def test_partition_of_the_virus_database(K, dev, virus):
    h, d, pat, full = virus
    assert h.N == 165
    _partition(d, pat, h.N, full, seeds=range(4))
    check_tiled(d, pat, h.N, 0, h.N, full, 64, 2)
    # a prefix shard is a handle like any other: its partial band
    p = K.DeviceDB(h, device=dev, prefix_shard=(1, 3))
    assert np.array_equal(p.all2all_rows_tiled(100, 165), p.all2all_dense()[tri(100): tri(165)])
    p.close()


def _band_tensor(d, lo, hi, dev):
    """the band in a torch tensor that held other values before (the buffer need not be zeroed)"""
    import torch
    t = torch.full((max(1, tri(hi) - tri(lo)),), -1, dtype=torch.int32, device=torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    d.all2all_rows_tiled_device(t.data_ptr(), lo, hi)
    return t


@pytest.mark.gpu
def test_refusals(K, S, dev, virus):
    h, d, pat, full = virus
    N = h.N
    lib = K.capi.lib()
    o = K.capi._opts(dev)
    assert lib.kmdb_all2all_rows_tiled_device(d._d, 3, 9, None, ctypes.byref(o)) != 0 and b"kmdb_all2all_rows_tiled_device: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows_tiled(d._d, 3, 9, None, ctypes.byref(o)) != 0 and b"kmdb_all2all_rows_tiled: null argument" in lib.kmdb_last_error()
    t = _band_tensor(d, 0, 2, dev)
    for call, who in ((lambda *a, **kw: d.all2all_rows_tiled(*a, **kw), "kmdb_all2all_rows_tiled"),
                      (lambda *a, **kw: d.all2all_rows_tiled_device(t.data_ptr(), *a, **kw), "kmdb_all2all_rows_tiled_device")):
        with pytest.raises(K.KmdbError, match=who + r": row_lo > row_hi \(9 > 3\)"):
            call(9, 3)
        with pytest.raises(K.KmdbError, match=who + ": row_hi 166 > the 165 samples"):
            call(3, N + 1)
        with pytest.raises(K.KmdbError, match=who + r": a band needs the whole pattern stream \(shard_count must be 1\)"):
            call(3, 9, shard=(0, 2))
        with pytest.raises(K.KmdbError, match=who + ": unknown bits in kmdb_opts.flags"):
            call(3, 9, flags=1 << 9)
        for cols in ("0", "63", "100", "40960", "64x", ""):
            with switches(cols), pytest.raises(K.KmdbError, match=who + ": KMDB_ROWS_TILE_COLS=.*a multiple of 64 from 64 to 40896"):
                call(3, 9)
        with switches(None, "0"), pytest.raises(K.KmdbError, match=who + ": KMDB_ROWS_TILE_HITS=0"):
            call(3, 9)
    # a call after a refusal still works, an empty band succeeds; the device form fills a buffer that held other values
    check_tiled(d, pat, N, 3, 9, full[tri(3): tri(9)])
    for lo, hi in ((7, 7), (0, 0), (0, 1), (N, N)):
        assert d.all2all_rows_tiled(lo, hi).size == 0
        d.all2all_rows_tiled_device(None, lo, hi)
        assert d.all2all_rows_tiled_stats()["band_cells"] == 0
    assert np.array_equal(_band_tensor(d, 100, 165, dev).cpu().numpy().view(np.uint32), full[tri(100): tri(165)])
    # a query shard
    q = K.DeviceDB(h, device=dev, query_shard=(0, 2))
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_tiled: not on a query shard"):
        q.all2all_rows_tiled(3, 9)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_tiled_device: not on a query shard"):
        q.all2all_rows_tiled_device(t.data_ptr(), 3, 9)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_sparse_filtered_banded: not on a query shard"):
        q.all2all_sparse_filtered_banded(10, [], None)
    q.close()
    check_tiled(d, pat, N, 100, 165, full[tri(100): tri(165)])


@pytest.mark.gpu
def test_a_band_beyond_the_device_is_refused(K, S, dev):
    """N = 500 000: all rows are 2^32 cells and more and half a terabyte — refused with the bytes; the last row alone (its first cell lies
    beyond 2^36) is computed"""
    pat, N = RC.huge_forest()
    d = _upload(K, S, pat, N, dev)
    t = _band_tensor(d, 0, 2, dev)
    with pytest.raises(K.KmdbError, match=r"kmdb_all2all_rows_tiled_device: the band is 124999750000 cells, 499999000000 bytes, beyond the \d+ bytes of device memory"):
        d.all2all_rows_tiled_device(t.data_ptr(), 0, N)
    lib = K.capi.lib()
    o = K.capi._opts(dev)
    one = np.zeros(1, np.uint32)
    assert lib.kmdb_all2all_rows_tiled(d._d, 0, N, one.ctypes.data, ctypes.byref(o)) != 0
    assert re.search(rb"kmdb_all2all_rows_tiled: the band is 124999750000 cells, 499999000000 bytes, beyond the \d+ bytes of free device memory", lib.kmdb_last_error())
    with pytest.raises(K.KmdbError, match=r"kmdb_all2all_sparse_filtered_banded: the band is 124999750000 cells"):
        d.all2all_sparse_filtered_banded(N, [], None)
    st = check_tiled(d, pat, N, N - 1, N, RC.band_definition(pat, N, N - 1, N))
    assert st["updates"] == 3 + 1 and tri(N - 1) > (1 << 36) and st["hits"] == 2 and st["jobs"] == len(range(0, N - 1, TC.DEFAULT_TILE_COLS))
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, the banded sparse call
# ------------------------------------------------------------------------------------------------------------------------------------
def _same_rows(got, want):
    assert got.n_rows == want.n_rows and got.nnz == want.nnz
    assert np.array_equal(got.row_ptr, want.row_ptr) and np.array_equal(got.col, want.col) and np.array_equal(got.val, want.val)
    assert (got.measure is None) == (want.measure is None)
    if want.measure is not None:
        assert np.array_equal(got.measure, want.measure)


@pytest.fixture(scope="module")
def sparse_wants(virus):
    h, d, pat, full = virus
    similar = d.all2all_sparse_filtered([("jaccard", 0.5, None)], h.sample_kmers)
    assert similar.nnz > 1
    cap = int(np.median(similar.val))                           # a maximum of common k-mers that cuts the similar pairs in two
    forms = {"plain": ([], None), "bounds": ([("jaccard", 0.5, None), ("num-kmers", None, cap)], None), "measure": ([], "mash")}
    return {k: (f, m, d.all2all_sparse_filtered(f, h.sample_kmers, measure=m)) for k, (f, m) in forms.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 7, 64, 165, 170])
def test_banded_sparse_call(virus, sparse_wants, R):
    h, d, pat, full = virus
    N = h.N
    for form, (filters, measure, want) in sparse_wants.items():
        assert want.nnz > 0 and (form != "bounds" or want.nnz < sparse_wants["plain"][2].nnz) and (form != "measure" or want.measure is not None), form
        got = d.all2all_sparse_filtered_banded(R, filters, h.sample_kmers, measure=measure)
        _same_rows(got, want)
        st = d.all2all_banded_stats()
        assert st["bands"] == -(-N // R) and st["max_band_bytes"] == 4 * max(tri(min(a + R, N)) - tri(a) for a in range(0, N, R)), st
        assert st["updates"] == RC.census(pat, 0, N)[1] and st["hits"] == TC.hits(pat, 0, N) and st["runs"] <= st["updates"], st
        assert st["peak_device_bytes"] > st["max_band_bytes"] and st["apply_ms"] > 0, st


@pytest.mark.gpu
def test_banded_sparse_call_edges(K, virus):
    h, d, pat, full = virus
    got = d.all2all_sparse_filtered_banded(40, [("jaccard", 2.0, None)], h.sample_kmers)
    assert got.nnz == 0 and got.n_rows == h.N and not got.row_ptr.any()
    with pytest.raises(K.KmdbError, match="kmdb_all2all_sparse_filtered_banded: band_rows is 0"):
        d.all2all_sparse_filtered_banded(0, [], h.sample_kmers)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_sparse_filtered_banded: null argument"):
        d.all2all_sparse_filtered_banded(10, [("jaccard", 0.5, None)], None)
    with pytest.raises(K.KmdbError, match=r"kmdb_all2all_sparse_filtered_banded: a band needs the whole pattern stream"):
        d.all2all_sparse_filtered_banded(10, [], h.sample_kmers, shard=(0, 2))
    with switches(64, 2):
        _same_rows(d.all2all_sparse_filtered_banded(50, [], None), d.all2all_sparse_filtered([], h.sample_kmers))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, front-end: byte for byte what the same command without -band-rows writes
# ------------------------------------------------------------------------------------------------------------------------------------
def _lines(path):
    return EC.read(path).splitlines(keepends=True)


@pytest.fixture()
def fe(dev, golden_dir, tmp_path):
    return (lambda n: os.path.join(golden_dir, n)), (lambda n: str(tmp_path / n))


VERBOSE_LINE = r"\[kmdb\] all2all rows tiled: rows (\d+) to (\d+), "      # (it may follow a progress message that has not ended its line)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [40, 1, 165, 1000])
def test_front_end_dense(fe, R):
    g, t = fe
    r = _cli("all2all", "-band-rows", str(R), g("virus_k18.db"), t("a.csv"), env={"KMDB_VERBOSE": "1"})
    assert EC.read(t("a.csv")) == EC.read(g("virus.k18.csv"))
    bands = [(int(a), int(b)) for a, b in re.findall(VERBOSE_LINE, r.stderr, re.M)]
    assert bands == [(a, min(a + R, 165)) for a in range(0, 165, R)], r.stderr          # one line per band


@pytest.mark.gpu
def test_front_end_sparse(fe):
    g, t = fe
    r = _cli("all2all", "-sparse", "-band-rows", "40", g("virus_k18.db"), t("a.csv"), env={"KMDB_VERBOSE": "1"})
    assert EC.read(t("a.csv")) == EC.read(g("virus.k18.sparse.csv"))
    assert len(re.findall(VERBOSE_LINE, r.stderr, re.M)) == 5
    full = _cli("all2all-sp", g("virus_k18.db"), t("full.csv"))
    for R in ("1", "165"):
        r = _cli("all2all-sp", "-band-rows", R, g("virus_k18.db"), t("b.csv"))
        assert EC.read(t("b.csv")) == EC.read(g("virus.k18.sparse.csv"))
        pairs = re.findall(r"^No\. saved pairs: (\d+)$", r.stderr, re.M)
        assert len(pairs) == 1 and pairs == re.findall(r"^No\. saved pairs: (\d+)$", full.stderr, re.M)       # the sum over the bands
    sw = ("-min", "jaccard:0.5", "-max", "num-kmers:20000")
    _cli("all2all-sp", *sw, g("virus_k18.db"), t("f.want"))
    _cli("all2all-sp", *sw, "-band-rows", "40", g("virus_k18.db"), t("f.csv"))
    assert EC.read(t("f.csv")) == EC.read(t("f.want")) and len(EC.read(t("f.csv"))) < len(EC.read(t("b.csv")))
    _cli("all2all", "-sparse", *sw, "-band-rows", "7", g("virus_k18.db"), t("f2.csv"))
    assert EC.read(t("f2.csv")) == EC.read(t("f.want"))


@pytest.mark.gpu
def test_front_end_distance(fe):
    g, t = fe
    r = _cli("all2all", "-distance", "jaccard", "-band-rows", "40", g("virus_k18.db"), t("j.csv"), env={"KMDB_VERBOSE": "1"})
    assert EC.read(t("j.csv")) == EC.read(g("virus.k18.csv.jaccard"))
    assert len(re.findall(VERBOSE_LINE, r.stderr, re.M)) == 5
    # two measures from every band, the sparse form with a bound, pieces of 150 cells: against the full run
    sw = ("-distance", "ani", "-distance", "min", "-min", "0.5")
    _cli("all2all-sp", *sw, g("virus_k18.db"), t("two.want"))
    _cli("all2all-sp", *sw, "-band-rows", "25", g("virus_k18.db"), t("two.got"), env={"KMDB_DISTANCE_CELLS_PER_PIECE": "150"})
    for suffix in (".ani", ".min"):
        want = EC.read(t("two.want" + suffix))
        assert len(want.splitlines()) == 166 and EC.read(t("two.got" + suffix)) == want, suffix
    assert not os.path.exists(t("two.got"))


@pytest.mark.gpu
def test_front_end_with_rows(fe):
    g, t = fe
    for form in ((), ("-sparse",), ("-distance", "jaccard")):
        _cli("all2all", *form, "-rows", "30:101", g("virus_k18.db"), t("want.csv"))
        r = _cli("all2all", *form, "-rows", "30:101", "-band-rows", "25", g("virus_k18.db"), t("got.csv"), env={"KMDB_VERBOSE": "1"})
        assert EC.read(t("got.csv")) == EC.read(t("want.csv")) and len(_lines(t("got.csv"))) >= 72, form
        assert [(int(a), int(b)) for a, b in re.findall(VERBOSE_LINE, r.stderr, re.M)] == [(30, 55), (55, 80), (80, 101)], (form, r.stderr)
    # an empty range: the header lines alone
    _cli("all2all", "-rows", "7:7", "-band-rows", "25", g("virus_k18.db"), t("e.csv"))
    assert _lines(t("e.csv")) == _lines(g("virus.k18.csv"))[:2]
    _cli("all2all-sp", "-rows", "7:7", "-band-rows", "25", g("virus_k18.db"), t("e2.csv"))
    assert _lines(t("e2.csv")) == _lines(g("virus.k18.sparse.csv"))[:2]


@pytest.mark.gpu
def test_front_end_rows_new(fe, golden_dir, tmp_path):
    g, t = fe
    root = MC.link_virus_data(golden_dir, str(tmp_path))
    want = _lines(g("virus.k18.csv"))
    r = _cli("all2all", "-from-samples", "-extend-from", g("virus_k18_part1.db"), "-rows", "new", "-band-rows", "20", g("virus.seqs.part2.list"), t("new.csv"),
             cwd=root, env={"KMDB_VERBOSE": "1"})
    assert _lines(t("new.csv")) == want[:2] + want[-65:]
    assert [(int(a), int(b)) for a, b in re.findall(VERBOSE_LINE, r.stderr, re.M)] == [(100, 120), (120, 140), (140, 160), (160, 165)], r.stderr


@pytest.mark.gpu
def test_front_end_rows_take_the_tiled_call_on_request(fe):
    g, t = fe
    for form in ((), ("-sparse",), ("-distance", "jaccard")):
        plain = _cli("all2all", *form, "-rows", "100:", g("virus_k18.db"), t("want.csv"), env={"KMDB_VERBOSE": "1"})
        tiled = _cli("all2all", *form, "-rows", "100:", g("virus_k18.db"), t("got.csv"), env={"KMDB_VERBOSE": "1", "KMDB_ROWS_TILED": "1"})
        assert EC.read(t("got.csv")) == EC.read(t("want.csv")) and len(_lines(t("got.csv"))) >= 66, form
        assert "[kmdb] all2all rows: " in plain.stderr and "all2all rows tiled" not in plain.stderr, form
        assert len(re.findall(VERBOSE_LINE, tiled.stderr, re.M)) == 1 and "[kmdb] all2all rows: " not in tiled.stderr, form
