"""all2all bands through the block-record pipeline: kmdb_all2all_rows_records_device / kmdb_all2all_rows_records /
kmdb_all2all_rows_records_stats_get (KMDB_HAS_ALL2ALL_ROWS_RECORDS), kmdb_all2all_sparse_filtered_banded_path and the front-end's
`all2all | all2all-sp -rows / -band-rows ... -band-path <tree|tiled|records>`.

DEFINITION of the call: bit for bit what kmdb_all2all_rows_device writes for the same arguments — the cells [tri(row_lo), tri(row_hi)) of
kmdb_all2all_dense_device.  Every device check holds the band against the flat-form definition in numpy (variant_cases.definition) AND against the
tree band call.  Every output buffer is a torch tensor of 3 tri(N) words filled with a sentinel; the band starts at word tri(N); the words in
front of it and behind it must still hold the sentinel after the call (a wrongly based write lands in allocated memory and fails the test)."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import all2all_rows_cases as RC
import all2all_rows_records_cases as RR
import variant_cases as VC
import wide_cases as W
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
HEADER = os.path.join(ROOT, "include", "kmdb_amd.h")
BUILD_DIR = os.path.join(ROOT, "kmer-db_amd", "build")
NEW_SYMBOLS = ("kmdb_all2all_rows_records_device", "kmdb_all2all_rows_records", "kmdb_all2all_rows_records_stats_get",
               "kmdb_all2all_sparse_filtered_banded_path", "kmdb_all2all_banded_records_stats_get")
SWITCHES = ("KMDB_K1N_MODE", "KMDB_ROW_MODE", "KMDB_BLOCK_WIDTH", "KMDB_SLICES", "KMDB_L2_MIN", "KMDB_L2", "KMDB_POOL_PERCENT", "KMDB_REC_PACKED",
            "KMDB_K1W_RUN", "KMDB_K1W_WAVES", "KMDB_NSEG", "KMDB_VERBOSE")
# the three record paths of test_wide_conformance.py's MODES
MODES = {"few streams": {}, "rows, no L2": dict(KMDB_ROW_MODE=1, KMDB_L2=0), "rows, L2 from 11": dict(KMDB_ROW_MODE=1, KMDB_L2_MIN=11)}
tri = RC.tri


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _cli(*args, cwd=None, ok=True, env=None):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, cwd=cwd, env=None if env is None else dict(os.environ, **env))
    if ok:
        assert r.returncode == 0, r.stderr
    return r


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_declared(K):
    src = _read(HEADER).decode()
    assert re.search(r"^#define KMDB_HAS_ALL2ALL_ROWS_RECORDS 1$", src, re.M)
    assert re.search(r"^#define KMDB_ABI_VERSION 8$", src, re.M)
    for i, name in enumerate(("KMDB_BAND_PATH_TILED", "KMDB_BAND_PATH_TREE", "KMDB_BAND_PATH_RECORDS")):
        assert re.search(r"^#define %s\s+%d$" % (name, i), src, re.M), name
    assert K.capi.BAND_PATHS == ("tiled", "tree", "records")
    L = ctypes.CDLL(K.lib_path())
    for name in NEW_SYMBOLS:
        assert name in K.capi.EXPORTS and hasattr(L, name), name
        assert re.search(r"^int\s+%s\(" % name, src, re.M), name
    ctype = {"c_ulong": "uint64_t", "c_uint": "uint32_t", "c_double": "double"}
    for struct, fields in (("kmdb_all2all_rows_records_stats", K.capi._All2allRowsRecordsStats._fields_),
                           ("kmdb_all2all_banded_records_stats", K.capi._All2allBandedRecordsStats._fields_)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        decl = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|uint32_t|double)\s+([^;]+);", body) for n in names.split(",")]
        assert decl == [(ctype[t.__name__], f) for f, t in fields], struct
    for meth in ("all2all_rows_records", "all2all_rows_records_device", "all2all_rows_records_stats", "all2all_banded_records_stats"):
        assert hasattr(K.DeviceDB, meth), meth
    import inspect
    assert "path" in inspect.signature(K.DeviceDB.all2all_sparse_filtered_banded).parameters


def test_null_arguments_are_refused_by_name(K):
    lib = K.capi.lib()
    assert lib.kmdb_all2all_rows_records_device(None, 0, 0, None, None) != 0 and b"kmdb_all2all_rows_records_device: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows_records(None, 0, 0, None, None) != 0 and b"kmdb_all2all_rows_records: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows_records_stats_get(None, None) != 0 and b"kmdb_all2all_rows_records_stats_get: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_sparse_filtered_banded_path(None, 5, 2, None, 0, None, -1, None, None) != 0
    assert b"kmdb_all2all_sparse_filtered_banded_path: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_banded_records_stats_get(None, None) != 0 and b"kmdb_all2all_banded_records_stats_get: null argument" in lib.kmdb_last_error()


def test_cli_refusals_by_name_and_usage(tmp_path):
    """refused before any file is read or any device touched: one ERROR line that names the switch, nothing written, the database (which does not
    exist) never mentioned; the refusals of -rows and -band-rows stay word for word"""
    db, out = str(tmp_path / "no_such.db"), str(tmp_path / "out.csv")
    for mode in ("all2all", "all2all-sp"):
        for args, words in (((mode, "-band-path", "records", db, out), ("-band-path goes with -rows", "-band-rows")),
                            ((mode, "-rows", "3:9", "-band-path", "fast", db, out), ("-band-path expects tree, tiled or records: fast",)),
                            ((mode, "-band-rows", "40", "-band-path", "", db, out), ("-band-path expects tree, tiled or records",)),
                            ((mode, "-band-rows", "40", db, out, "-band-path"), ("-band-path expects tree, tiled or records",)),
                            ((mode, "-rows", "3:9", "-band-path", "records", "-gpus", "2", db, out),
                             ("-rows does not go with -gpus <N>: a band is computed on one device from the whole pattern tree",)),
                            ((mode, "-band-rows", "40", "-band-path", "records", "-sample-rows", "jaccard:3", db, out),
                             ("-band-rows does not go with -sample-rows: a pair is offered to both its samples, so a band of rows does not hold a sample's candidates",)),
                            ((mode, "-rows", "3:9", "-band-path", "records", "-phylip-out", "-distance", "mash", db, out),
                             ("-rows does not go with -phylip-out: a phylip table is a whole triangle",))):
            r = _cli(*args, ok=False)
            assert r.returncode not in (0, -11, -6), (args, r.stderr)
            err = [ln for ln in r.stderr.splitlines() if ln.startswith("ERROR: ")]
            assert len(err) == 1 and all(w in err[0] for w in words), (args, r.stderr)
            assert "no_such" not in r.stderr and "Loading" not in r.stderr, (args, r.stderr)
            assert not os.path.exists(out), args
    for mode in ("new2all", "one2all", "all2all-parts", "build", "distance", "minhash"):
        r = _cli(mode, "-band-path", "records", db, out, ok=False)
        assert r.returncode != 0 and "-band-path applies to all2all and all2all-sp" in r.stderr and "no_such" not in r.stderr, (mode, r.stderr)
    # a well-formed run goes on to the file, which is not there
    for path in ("tree", "tiled", "records"):
        r = _cli("all2all", "-rows", "3:9", "-band-path", path, db, out, ok=False)
        assert r.returncode != 0 and "no_such.db" in r.stderr, path
    usage = _cli().stderr
    assert "-band-path <tree|tiled|records>" in usage and "all2all / all2all-sp -band-path <tree|tiled|records>:" in usage


@pytest.mark.parametrize("width", [32, 33, 50, 64])
def test_the_window_against_brute_force(width):
    """which cells of tile (X, Y) fall into [row_lo, row_hi) and where: the numpy restatement of the write-back (the 64-bit form of k2_run and of the
    second level, and the slice kernel's base + 32-bit lane offset) against a cell-by-cell walk, for bands that start and end on a block edge, one
    before it, one after it and inside a single block; over all tiles of a band the offsets are exactly 0 .. cells - 1, each once.
    (Host arithmetic only: this pins the statement of the window, not the kernels — those are held by the device tests below, whose bands start
    and end before, on, after and inside a block edge.)"""
    for N in (3 * width + 1, 4 * width - 1):
        NB = (N + width - 1) // width
        for lo, hi in RR.window_bands(width, N):
            xlo, xhi = RR.block_rows(width, lo, hi)
            assert xlo * width <= lo < (xlo + 1) * width and xhi * width < hi <= (xhi + 1) * width
            seen = []
            for X in range(NB):
                for Y in range(X + 1):
                    r, c, off = RR.tile_window(width, N, lo, hi, X, Y)
                    want = RR.brute_window(width, N, lo, hi, X, Y)
                    assert set(zip(r.tolist(), c.tolist(), off.tolist())) == want, (N, lo, hi, X, Y)
                    assert (not want) or not RR.culled(width, lo, hi, X)
                    if X == Y:
                        r2, c2, off2 = RR.slice_tile_window(width, N, lo, hi, X)
                        assert set(zip(r2.tolist(), c2.tolist(), off2.tolist())) == want, (N, lo, hi, X)
                    seen.append(off)
            seen = np.sort(np.concatenate(seen))
            assert np.array_equal(seen, np.arange(tri(hi) - tri(lo))), (N, lo, hi)


def test_band_instantiations_spill_nothing():
    """the compiler's resource remarks of a2a_blocks.hip: the four band instantiations of the apply stage exist, without scratch and without a
    spilled register"""
    res = os.path.join(BUILD_DIR, "a2a_blocks.resources.txt")
    assert os.path.exists(res), ("%s is missing: the build writes it (make -C kmer-db_amd, or __graft_entry__.build()) from the compiler's "
                                 "-Rpass-analysis=kernel-resource-usage remarks" % res)
    found, cur = {}, None
    with open(res, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.match(r"_ZN12_GLOBAL__N_1\d+(k2d_band_kernel|(?:k2_jobs_kernel|k2_apply_kernel|l2_join_apply_kernel)ILb1EE)", m.group(1))
                cur = found.setdefault(k.group(1), {}) if k else None
                continue
            m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
    assert set(found) == {"k2d_band_kernel", "k2_jobs_kernelILb1EE", "k2_apply_kernelILb1EE", "l2_join_apply_kernelILb1EE"}, sorted(found)
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


@pytest.fixture
def env(monkeypatch):
    """set(name=value, ...) replaces ALL of the engine's switches by the ones given (None: unset); they are read when a handle is made"""
    def set_(**kw):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in kw.items():
            assert name in SWITCHES, name
            if value is not None:
                monkeypatch.setenv(name, str(value))
    set_()
    return set_


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


def records_band(d, N, lo, hi, dev, flags=0):
    """one call of kmdb_all2all_rows_records_device into the middle of a sentinel buffer of 3 tri(N) words; the band, and the call's stats"""
    import torch
    T = max(tri(N), 1)
    cells = tri(hi) - tri(lo)
    buf = torch.full((3 * T,), RR.SENTINEL - (1 << 32), dtype=torch.int32, device=torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    d.all2all_rows_records_device(buf.data_ptr() + 4 * T, lo, hi, flags=flags)
    torch.cuda.synchronize(dev)
    sent = RR.SENTINEL - (1 << 32)
    assert bool((buf[:T] == sent).all()), "band [%d, %d): words in front of the band were written" % (lo, hi)
    assert bool((buf[T + cells:] == sent).all()), "band [%d, %d): words behind the band were written" % (lo, hi)
    got = buf[T: T + cells].cpu().numpy().view(np.uint32)
    st = d.all2all_rows_records_stats()
    assert st["band_cells"] == cells, (lo, hi, st)
    return got, st


def check_band(d, N, lo, hi, exp, dev, tree=True, flags=0):
    """the records band against the definition and against kmdb_all2all_rows_device (through its host variant); the stats' invariants"""
    got, st = records_band(d, N, lo, hi, dev, flags)
    assert got.size == exp.size and np.array_equal(got, exp), "band [%d, %d): %d of %d cells differ from the definition" % (lo, hi, int((got != exp).sum()), exp.size)
    if tree:
        assert np.array_equal(got, d.all2all_rows(lo, hi)), "band [%d, %d) differs from kmdb_all2all_rows" % (lo, hi)
    if exp.size:
        assert st["path"] in (1, 2), st
        if st["path"] == 1:
            w = st["width"]
            assert (st["x_lo"], st["x_hi"]) == (lo // w, (hi - 1) // w) and st["units_run"] <= st["units_total"], (lo, hi, st)
            assert st["units_total"] == st["jobs_total"] + st["runs_total"] + st["slices_total"] + st["tiles_total"], st
            assert st["units_run"] == st["jobs_run"] + st["runs_run"] + st["slices_run"] + st["tiles_run"], st
            assert st["peak_device_bytes"] >= 4 * exp.size and st["kernel_ms"] > 0 and st["slices"] >= 1, st
    return got, st


def _partition(d, N, full, dev, seeds=range(3)):
    for seed in seeds:
        cuts = RC.seeded_cuts(N, 2000 + seed, 3 + 2 * seed)
        parts = [check_band(d, N, a, b, full[tri(a): tri(b)], dev)[0] for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts), full), cuts


@pytest.mark.gpu
@pytest.mark.parametrize("k1n", [0, 2])
@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("width", VC.WIDTHS)
def test_edge_forests(K, S, dev, env, width, rows, k1n):
    """variant_cases.edge_forest at both edge sizes (weights either side of 127 | 128 and of 2^32 are in them) under KMDB_ROW_MODE x KMDB_K1N_MODE, with
    KMDB_NSEG default and 64: a seeded partition into bands, every one-row band from width - 1 to width + 1 and from 2 width - 1 to N, and [0, N)
    against all2all_dense"""
    for N in VC.edge_sizes(width):
        pat, full = RR.edge_case(width, N)
        _, view = VC.make_view(K, S, pat, N)
        for nseg in (None, 64):
            env(KMDB_BLOCK_WIDTH=width, KMDB_ROW_MODE=rows, KMDB_K1N_MODE=k1n, KMDB_NSEG=nseg)
            d = K.DeviceDB(view, device=dev)
            _partition(d, N, full, dev, seeds=range(1 if nseg else 2))
            for lo, hi in RR.one_row_bands(width, N):
                _, st = check_band(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
                assert st["path"] == 1 and st["width"] == width, st
            got, st = check_band(d, N, 0, N, full, dev)
            assert np.array_equal(got, d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)) and st["units_run"] == st["units_total"] > 0, st
            d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k1n", [0, 2])
@pytest.mark.parametrize("rows", [0, 1])
def test_light_forest(K, S, dev, env, rows, k1n):
    """variant_cases.light_forest: diagonal tiles that get first-block records of the matrix-core step only"""
    width, N = 50, 4 * 50 - 1
    pat = VC.light_forest(width, N)
    full = VC.definition(pat, N)
    env(KMDB_BLOCK_WIDTH=width, KMDB_ROW_MODE=rows, KMDB_K1N_MODE=k1n)
    d = _upload(K, S, pat, N, dev)
    _partition(d, N, full, dev)
    for lo, hi in RR.block_bands(width, N) + RR.one_row_bands(width, N)[::7]:
        check_band(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_wide_forest(K, dev, env, mode):
    """wide_cases.wide_forest (width 32) under few streams / rows without the second level / rows with it from 11 blocks: one block row, two, a row
    range inside one block, all of it"""
    c = W.case("wide", 32, False)
    N, full = c["N"], c["exp"]
    _, view = VC.make_view(K, importlib.import_module("kmerdb_amd.synth"), c["pat"], N)
    env(KMDB_BLOCK_WIDTH=32, **MODES[mode])
    d = K.DeviceDB(view, device=dev)
    for lo, hi in RR.block_bands(32, N) + [(N - 1, N), (31, 33)]:
        _, st = check_band(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
        assert st["path"] == 1 and (st["tiles_total"] > 0) == (mode == "rows, L2 from 11"), (mode, st)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_join_forest(K, dev, env, mode):
    """wide_cases.join_forest: more than L2_QCAP matches in the tiles (7, 3), (3, 3), (7, 7), weights of one to five digits, cells that wrap"""
    c = W.case("join")
    N, full = c["N"], c["exp"]
    _, view = VC.make_view(K, importlib.import_module("kmerdb_amd.synth"), c["pat"], N)
    env(KMDB_BLOCK_WIDTH=32, **MODES[mode])
    d = K.DeviceDB(view, device=dev)
    for lo, hi in ((3 * 32, 4 * 32), (7 * 32, 9 * 32), (7 * 32 + 3, 7 * 32 + 9), (0, N)):
        _, st = check_band(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
        if mode == "rows, L2 from 11":
            assert 0 < st["tiles_run"] <= st["tiles_total"], st
            assert (st["tiles_run"] == st["tiles_total"]) == ((lo, hi) == (0, N)), st
    d.close()


@pytest.mark.gpu
def test_a_band_outside_every_joined_tile_runs_no_second_level_tile(K, S, dev, env):
    """join_forest's 40 blocks all lie in some joined node's list, so every block row has a second-level tile with two lists: the forest is taken with
    two more block rows, 40 and 41, that hold narrow patterns only (all2all_rows_records_cases.extended_join_forest).  A band over them runs zero
    second-level tiles and is exact; a band over block row 3 runs some."""
    pat, N = RR.extended_join_forest()
    full = VC.definition(pat, N)
    env(KMDB_BLOCK_WIDTH=32, KMDB_ROW_MODE=1, KMDB_L2_MIN=11)
    d = _upload(K, S, pat, N, dev)
    _, st = check_band(d, N, 40 * 32, N, full[tri(40 * 32):], dev)
    assert st["tiles_total"] > 0 and st["tiles_run"] == 0 and st["units_run"] > 0, st
    _, st = check_band(d, N, 40 * 32 + 5, 41 * 32 + 3, full[tri(40 * 32 + 5): tri(41 * 32 + 3)], dev)
    assert st["tiles_total"] > 0 and st["tiles_run"] == 0, st
    _, st = check_band(d, N, 3 * 32, 4 * 32, full[tri(3 * 32): tri(4 * 32)], dev)
    assert 1 <= st["tiles_run"] <= 4, st                          # (3, 0) .. (3, 3)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [None, 0])
@pytest.mark.parametrize("rowmode", [0, 1])
@pytest.mark.parametrize("n", [16384, 16385])
def test_stream_jobs(K, dev, env, n, rowmode, packed):
    """wide_cases.stream_forest: 16 384 | 16 385 records of stream (1, 0) — one job or two: a band that holds block row 1, and one that does not"""
    c = W.case("stream", n, bool(rowmode))
    N, full = c["N"], c["exp"]
    _, view = VC.make_view(K, importlib.import_module("kmerdb_amd.synth"), c["pat"], N)
    env(KMDB_BLOCK_WIDTH=32, KMDB_ROW_MODE=rowmode, KMDB_REC_PACKED=packed, KMDB_K1W_WAVES=1)
    d = K.DeviceDB(view, device=dev)
    _, inside = check_band(d, N, 32, 64, full[tri(32): tri(64)], dev)
    _, outside = check_band(d, N, 64, N, full[tri(64): tri(N)], dev)
    _, whole = check_band(d, N, 0, N, full, dev)
    parts = 1 if n == 16384 else 2
    assert inside["jobs_total"] == outside["jobs_total"] == whole["jobs_total"] == whole["jobs_run"], (inside, outside, whole)
    assert inside["jobs_run"] >= parts and outside["jobs_run"] <= whole["jobs_run"] - parts, (inside, outside, whole)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [0, 1])
def test_a_warm_handle_serves_whole_calls_and_band_calls(K, S, dev, env, rows):
    """whole call, band call, whole call, band call on one handle: all four equal their definitions, no call after the first measures its launch
    sizes, the whole calls' n_records do not move and the band calls emit as many records"""
    width, N = 50, 4 * 50 - 1
    pat, full = RR.edge_case(width, N)
    env(KMDB_BLOCK_WIDTH=width, KMDB_ROW_MODE=rows)
    d = _upload(K, S, pat, N, dev)
    NF = K.capi.FLAG_NO_FALLBACK
    assert np.array_equal(d.all2all_dense(flags=NF), full)
    first = d.stats()
    assert first["sized_call"] == 1 and first["n_records"] > 0
    # (tree=False: the sequence on the handle is exactly whole, band, whole, band — no other call in between; the same bands are held to the tree call
    # on the second handle below and in test_edge_forests)
    _, b1 = check_band(d, N, 60, 130, full[tri(60): tri(130)], dev, tree=False, flags=NF)
    assert np.array_equal(d.all2all_dense(flags=NF), full)
    third = d.stats()
    _, b2 = check_band(d, N, 149, N, full[tri(149):], dev, tree=False, flags=NF)
    assert b1["sized_call"] == 0 and third["sized_call"] == 0 and b2["sized_call"] == 0, (b1, third, b2)
    assert third["n_records"] == first["n_records"] == b1["records"] == b2["records"], (first, b1, third, b2)
    d.close()
    # and the other way round: a handle whose first call is a band call
    d = _upload(K, S, pat, N, dev)
    _, b0 = check_band(d, N, 60, 130, full[tri(60): tri(130)], dev, flags=NF)
    assert b0["sized_call"] == 1
    assert np.array_equal(d.all2all_dense(flags=NF), full) and d.stats()["sized_call"] == 0
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [0, 1])
def test_slices(K, S, dev, env, rows):
    """KMDB_SLICES=3: every slice of the pattern stream adds into the same band"""
    width, N = 50, 4 * 50 - 1
    pat, full = RR.edge_case(width, N)
    _, view = VC.make_view(K, S, pat, N)
    env(KMDB_BLOCK_WIDTH=width, KMDB_ROW_MODE=rows, KMDB_SLICES=3)
    d = K.DeviceDB(view, device=dev)
    for lo, hi in RR.block_bands(width, N) + [(49, 51)]:
        _, st = check_band(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
        assert st["slices"] == 3 and st["path"] == 1, st
    d.close()


@pytest.mark.gpu
def test_small_pools(K, S, dev, env, capfd):
    """KMDB_POOL_PERCENT=1 on a collection whose records overflow the smallest pools of the many-streams path several times over (1200 samples in
    clades of 50, row mode): the pools are enlarged and the call is repeated from a band zeroed again — the band's bytes only: the sentinel words
    around it stay (records_band checks them).  The reference is the whole call of a handle with pools of the usual size."""
    import torch
    rows = 1
    N = 1200
    g, pat = S.synth_database(N, 50, 4000, k=18, seed=5, device=torch.device("cuda", dev))
    _, view = VC.make_view(K, S, pat, N)
    env(KMDB_BLOCK_WIDTH=32, KMDB_ROW_MODE=rows)
    d = K.DeviceDB(view, device=dev)
    full = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
    d.close()
    assert full.any()
    env(KMDB_BLOCK_WIDTH=32, KMDB_ROW_MODE=rows, KMDB_POOL_PERCENT=1, KMDB_VERBOSE=1)
    d = K.DeviceDB(view, device=dev)
    capfd.readouterr()
    _, st = check_band(d, N, 400, 500, full[tri(400): tri(500)], dev)
    err = capfd.readouterr().err
    assert re.search(r"too small|at its limit", err), err[-2000:]
    assert st["path"] == 1 and st["sized_call"] == 1, st
    for lo, hi in ((32, 64), (1150, N), (0, 40)):
        check_band(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k1n", [0, 2])
def test_the_cull(K, S, dev, env, k1n):
    """row mode, four block rows: a band of one block row runs fewer apply units than the call meets, [0, N) runs them all"""
    width, N = 32, 4 * 32 - 1
    pat, full = RR.edge_case(width, N)
    env(KMDB_BLOCK_WIDTH=width, KMDB_ROW_MODE=1, KMDB_K1N_MODE=k1n)
    d = _upload(K, S, pat, N, dev)
    _, whole = check_band(d, N, 0, N, full, dev)
    assert whole["units_run"] == whole["units_total"] > 0, whole
    for X in range(4):
        lo, hi = X * width, min((X + 1) * width, N)
        _, st = check_band(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
        assert st["units_total"] == whole["units_total"] and 0 < st["units_run"] < st["units_total"], (X, st)
        assert (st["x_lo"], st["x_hi"]) == (X, X)
    d.close()


@pytest.mark.gpu
def test_partition_of_the_virus_database(virus, dev):
    h, d, pat, full = virus
    assert h.N == 165 and np.array_equal(full, VC.definition(pat, h.N))
    _partition(d, h.N, full, dev, seeds=range(5))


@pytest.mark.gpu
def test_partition_of_a_clade_collection(K, S, dev):
    N = 257
    g, pat = S.synth_database(N, 13, 1500, k=18, seed=7 + N, device="cpu")
    d = _upload(K, S, pat, N, dev)
    full = d.all2all_dense()
    assert np.array_equal(full, VC.definition(pat, N))
    _partition(d, N, full, dev, seeds=range(5))
    d.close()


@pytest.mark.gpu
def test_partition_on_a_handed_over_builder(K, S, dev):
    """a handle from Builder.finish_device against the upload of the finished image"""
    n, k = 40, 18
    g = S.CladeGenomes(n, 8, 6000, seed=11)
    names = [g.name(i) for i in range(n)]
    lists = [S.kmers_of(g.sample(i), k, 1.0).cpu().numpy().view(np.uint64).copy() for i in range(n)]
    b1, b2 = K.Builder(k, 1.0), K.Builder(k, 1.0)
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
    assert full.any()
    _partition(d2, d2.N, full, dev)
    d1.close()
    d2.close()


def _band_tensor(d, lo, hi, dev):
    import torch
    t = torch.full((max(1, tri(hi) - tri(lo)),), -1, dtype=torch.int32, device=torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    d.all2all_rows_records_device(t.data_ptr(), lo, hi)
    return t


@pytest.mark.gpu
def test_consumers_sparse(K, dev, virus):
    h, d, pat, full = virus
    lo, hi = 100, 165
    t = _band_tensor(d, lo, hi, dev)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), full[tri(lo): tri(hi)])
    for filters in ([], [("jaccard", 0.9, None)]):
        want = d.all2all_sparse_filtered(filters, h.sample_kmers)
        t = _band_tensor(d, lo, hi, dev)                        # (after a whole call: the tile flags are the whole call's, the band call's replace them)
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
    band = K.Distance(measure, h.k, h.sample_kmers, triangle=True, device=dev)
    band.take_cells(t.data_ptr(), lo, h.names)
    got = band.matrix_rows(lo, hi)
    band.close()
    assert len(want) > 1000 and got == want


def _same_rows(got, want):
    assert got.n_rows == want.n_rows and got.nnz == want.nnz
    assert np.array_equal(got.row_ptr, want.row_ptr) and np.array_equal(got.col, want.col) and np.array_equal(got.val, want.val)
    assert (got.measure is None) == (want.measure is None)
    if want.measure is not None:
        assert np.array_equal(got.measure, want.measure)


@pytest.fixture(scope="module")
def sparse_wants(virus):
    """kmdb_all2all_sparse_filtered's rows in three forms — no filter, two bounds that cut the similar pairs in two, a measure — computed once"""
    h, d, pat, full = virus
    similar = d.all2all_sparse_filtered([("jaccard", 0.5, None)], h.sample_kmers)
    assert similar.nnz > 1
    cap = int(np.median(similar.val))
    forms = {"plain": ([], None), "bounds": ([("jaccard", 0.5, None), ("num-kmers", None, cap)], None), "measure": ([], "mash")}
    return {k: (f, m, d.all2all_sparse_filtered(f, h.sample_kmers, measure=m)) for k, (f, m) in forms.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 7, 64, 165, 170])
def test_banded_sparse_call_on_the_records_path(K, virus, sparse_wants, R):
    h, d, pat, full = virus
    N = h.N
    for form, (filters, measure, want) in sparse_wants.items():
        assert want.nnz > 0 and (form != "bounds" or want.nnz < sparse_wants["plain"][2].nnz) and (form != "measure" or want.measure is not None), form
        got = d.all2all_sparse_filtered_banded(R, filters, h.sample_kmers, measure=measure, path="records")
        _same_rows(got, want)
        st, rs = d.all2all_banded_stats(), d.all2all_banded_records_stats()
        assert st["bands"] == -(-N // R) and st["max_band_bytes"] == 4 * max(tri(min(a + R, N)) - tri(a) for a in range(0, N, R)), st
        assert rs["bands"] == st["bands"], (st, rs)
        assert 0 < rs["units_run"] <= rs["units_total"] and rs["ms"] > 0, rs
    # the other two paths by name and by number, and what is refused
    _same_rows(d.all2all_sparse_filtered_banded(R, [], h.sample_kmers, path="tree"), sparse_wants["plain"][2])
    _same_rows(d.all2all_sparse_filtered_banded(R, [], h.sample_kmers, path=0), sparse_wants["plain"][2])
    with pytest.raises(K.KmdbError, match="kmdb_all2all_sparse_filtered_banded_path: unknown path 7"):
        d.all2all_sparse_filtered_banded(R, [], h.sample_kmers, path=7)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_sparse_filtered_banded_path: band_rows is 0"):
        d.all2all_sparse_filtered_banded(0, [], h.sample_kmers, path="records")


@pytest.mark.gpu
def test_refusals(K, S, dev, env, virus):
    h, d, pat, full = virus
    N = h.N
    lib = K.capi.lib()
    o = K.capi._opts(dev)
    assert lib.kmdb_all2all_rows_records_device(d._d, 3, 9, None, ctypes.byref(o)) != 0
    assert b"kmdb_all2all_rows_records_device: null argument" in lib.kmdb_last_error()
    assert lib.kmdb_all2all_rows_records(d._d, 3, 9, None, ctypes.byref(o)) != 0 and b"kmdb_all2all_rows_records: null argument" in lib.kmdb_last_error()
    t = _band_tensor(d, 0, 2, dev)
    for call, who in ((lambda *a, **kw: d.all2all_rows_records(*a, **kw), "kmdb_all2all_rows_records"),
                      (lambda *a, **kw: d.all2all_rows_records_device(t.data_ptr(), *a, **kw), "kmdb_all2all_rows_records_device")):
        with pytest.raises(K.KmdbError, match=who + r": row_lo > row_hi \(9 > 3\)"):
            call(9, 3)
        with pytest.raises(K.KmdbError, match=who + ": row_hi 166 > the 165 samples"):
            call(3, N + 1)
        with pytest.raises(K.KmdbError, match=who + r": a band needs the whole pattern stream \(shard_count must be 1\)"):
            call(3, 9, shard=(0, 2))
        with pytest.raises(K.KmdbError, match=who + ": unknown bits in kmdb_opts.flags"):
            call(3, 9, flags=1 << 9)
    # a call after a refusal still works, an empty band succeeds and writes nothing
    check_band(d, N, 3, 9, full[tri(3): tri(9)], dev)
    for lo, hi in ((7, 7), (0, 0), (0, 1), (N, N)):
        assert d.all2all_rows_records(lo, hi).size == 0
        d.all2all_rows_records_device(None, lo, hi)
        st = d.all2all_rows_records_stats()
        assert st["band_cells"] == 0 and st["path"] == 0, st
        got, _ = records_band(d, N, lo, hi, dev)
        assert got.size == 0
    assert np.array_equal(d.all2all_rows_records(100, 165), full[tri(100): tri(165)])
    # a query shard
    q = K.DeviceDB(h, device=dev, query_shard=(0, 2))
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_records: not on a query shard"):
        q.all2all_rows_records(3, 9)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_records_device: not on a query shard"):
        q.all2all_rows_records_device(t.data_ptr(), 3, 9)
    q.close()
    # a prefix shard is a handle like any other: its partial band
    p = K.DeviceDB(h, device=dev, prefix_shard=(1, 3))
    assert np.array_equal(p.all2all_rows_records(100, 165), p.all2all_dense()[tri(100): tri(165)])
    p.close()
    # a handle whose narrow kernel writes the matrix itself
    env(KMDB_K1N_MODE=1)
    m1 = K.DeviceDB(h, device=dev)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_records: this handle was made under KMDB_K1N_MODE=1"):
        m1.all2all_rows_records(3, 9)
    import torch
    t9 = torch.full((tri(9) - tri(3),), 77, dtype=torch.int32, device=torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_records_device: this handle was made under KMDB_K1N_MODE=1"):
        m1.all2all_rows_records_device(t9.data_ptr(), 3, 9)
    torch.cuda.synchronize(dev)
    assert bool((t9 == 77).all()), "a refused call wrote into the caller's buffer"
    assert np.array_equal(m1.all2all_dense(), full)
    m1.close()
    env()
    # a band beyond the device
    pat2, N2 = RC.huge_forest()
    big = _upload(K, S, pat2, N2, dev)
    with pytest.raises(K.KmdbError, match=r"kmdb_all2all_rows_records_device: the band is 124999750000 cells, 499999000000 bytes, beyond the \d+ bytes of device memory"):
        big.all2all_rows_records_device(t.data_ptr(), 0, N2)
    one = np.zeros(1, np.uint32)
    assert lib.kmdb_all2all_rows_records(big._d, 0, N2, one.ctypes.data, ctypes.byref(o)) != 0
    assert re.search(rb"kmdb_all2all_rows_records: the band is 124999750000 cells, 499999000000 bytes, beyond the \d+ bytes of free device memory", lib.kmdb_last_error())
    big.close()


@pytest.mark.gpu
def test_a_tree_deeper_than_the_chain_table_takes_the_fallback(K, S, dev):
    """a root path of 4097 nodes: the pipeline cannot take the database — the band comes from kmdb_all2all_rows_device and the stats say so; with
    KMDB_FLAG_NO_FALLBACK the call fails with the reason"""
    pat, N = RC.deep_forest()
    d = _upload(K, S, pat, N, dev)
    exp = RC.band_definition(pat, N, 4090, 4100)
    got, st = check_band(d, N, 4090, 4100, exp, dev)
    assert st["path"] == 2 and st["units_total"] == 0 and d.fallback_reason() != "", (st, d.fallback_reason())
    assert np.array_equal(d.all2all_rows_records(4090, 4100), exp)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_records: block-record pipeline unavailable: .+"):
        d.all2all_rows_records(4090, 4100, flags=K.capi.FLAG_NO_FALLBACK)
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, front-end: -band-path records against the reference's goldens and against the same command without the switch, byte for byte
# ------------------------------------------------------------------------------------------------------------------------------------
def _lines(path):
    return _read(path).splitlines(keepends=True)


@pytest.fixture()
def fe(dev, golden_dir, tmp_path):
    return (lambda n: os.path.join(golden_dir, n)), (lambda n: str(tmp_path / n))


REC = ("-band-path", "records")


@pytest.mark.gpu
def test_front_end_dense(fe):
    g, t = fe
    db = g("virus_k18.db")
    want = _lines(g("virus.k18.csv"))
    assert len(want) == 167
    r = _cli("all2all", "-rows", "100:", *REC, db, t("a.csv"), env={"KMDB_VERBOSE": "1"})
    assert _lines(t("a.csv")) == want[:2] + want[102:167]
    m = re.search(r"\[kmdb\] all2all rows records: rows 100 to 165, (\d+) cells, block records, block rows (\d+) to (\d+) of width (\d+), (\d+) records, "
                  r"apply units run / total (\d+) / (\d+)", r.stderr)
    assert m and int(m.group(1)) == tri(165) - tri(100) and int(m.group(2)) == 100 // int(m.group(4)) and 0 < int(m.group(6)) <= int(m.group(7)), r.stderr
    _cli("all2all", "-rows", "100:", db, t("a0.csv"))
    assert _read(t("a.csv")) == _read(t("a0.csv"))
    r = _cli("all2all", "-band-rows", "40", *REC, db, t("b.csv"), env={"KMDB_VERBOSE": "1"})
    assert _read(t("b.csv")) == _read(g("virus.k18.csv")) and r.stderr.count("[kmdb] all2all rows records: rows ") == 5
    _cli("all2all", "-band-rows", "40", db, t("b0.csv"))
    assert _read(t("b.csv")) == _read(t("b0.csv"))
    _cli("all2all", "-rows", "30:131", "-band-rows", "7", *REC, db, t("c.csv"))
    assert _lines(t("c.csv")) == want[:2] + want[32:133]
    _cli("all2all", "-rows", "7:7", *REC, db, t("d.csv"))
    assert _lines(t("d.csv")) == want[:2]
    for path in ("tree", "tiled"):
        _cli("all2all", "-rows", "100:", "-band-path", path, db, t(path + ".csv"))
        assert _read(t(path + ".csv")) == _read(t("a.csv")), path


@pytest.mark.gpu
def test_front_end_sparse(fe):
    g, t = fe
    db = g("virus_k18.db")
    want = _lines(g("virus.k18.sparse.csv"))
    assert len(want) == 167
    _cli("all2all", "-sparse", "-rows", "100:", *REC, db, t("a.csv"))
    assert _lines(t("a.csv")) == want[:2] + want[102:167]
    _cli("all2all-sp", "-band-rows", "33", *REC, db, t("b.csv"))
    assert _read(t("b.csv")) == _read(g("virus.k18.sparse.csv"))
    _cli("all2all-sp", "-rows", "20:150", "-band-rows", "33", *REC, db, t("c.csv"))
    assert _lines(t("c.csv")) == want[:2] + want[22:152]
    sw = ("-min", "jaccard:0.5", "-max", "num-kmers:20000")
    _cli("all2all-sp", *sw, "-rows", "40:120", db, t("f.want"))
    _cli("all2all-sp", *sw, "-rows", "40:120", *REC, db, t("f.csv"))
    assert _read(t("f.csv")) == _read(t("f.want")) and len(_read(t("f.csv"))) > 100
    _cli("all2all", "-sparse", *sw, "-band-rows", "50", db, t("g.want"))
    _cli("all2all", "-sparse", *sw, "-band-rows", "50", *REC, db, t("g.csv"))
    assert _read(t("g.csv")) == _read(t("g.want"))


@pytest.mark.gpu
def test_front_end_distance(fe):
    g, t = fe
    db = g("virus_k18.db")
    want = _lines(g("virus.k18.csv.jaccard"))
    assert len(want) == 166
    _cli("all2all", "-distance", "jaccard", "-rows", "100:", *REC, db, t("j.csv"))
    assert _lines(t("j.csv")) == want[:1] + want[101:166]
    _cli("all2all", "-distance", "jaccard", "-band-rows", "48", *REC, db, t("k.csv"))
    assert _read(t("k.csv")) == _read(g("virus.k18.csv.jaccard"))
    sw = ("-distance", "ani", "-distance", "min", "-min", "0.5")
    _cli("all2all-sp", *sw, "-rows", "30:101", "-band-rows", "25", db, t("two.want"))
    _cli("all2all-sp", *sw, "-rows", "30:101", "-band-rows", "25", *REC, db, t("two.got"))
    for suffix in (".ani", ".min"):
        assert len(_lines(t("two.want" + suffix))) == 72 and _read(t("two.got" + suffix)) == _read(t("two.want" + suffix)), suffix


@pytest.mark.gpu
def test_front_end_rows_new(fe, golden_dir, tmp_path):
    """-from-samples -extend-from <old.db> -rows new: the rows of the samples added, from the records call"""
    g, t = fe
    root = str(tmp_path)
    src, dst = os.path.join(golden_dir, "test", "virus", "data"), os.path.join(root, "test", "virus", "data")
    os.makedirs(dst)
    for fn in os.listdir(src):
        if not fn.endswith(".minhash"):
            os.symlink(os.path.join(src, fn), os.path.join(dst, fn))
    want = _lines(g("virus.k18.csv"))
    _cli("all2all", "-from-samples", "-extend-from", g("virus_k18_part1.db"), "-rows", "new", *REC, g("virus.seqs.part2.list"), t("new.csv"), cwd=root)
    assert _lines(t("new.csv")) == want[:2] + want[-65:]
    sp = _lines(g("virus.k18.sparse.csv"))
    _cli("all2all-sp", "-from-samples", "-extend-from", g("virus_k18_part1.db"), "-rows", "new", "-band-rows", "20", *REC, g("virus.seqs.part2.list"), t("new.sp.csv"),
         cwd=root)
    assert _lines(t("new.sp.csv")) == sp[:2] + sp[-65:]
