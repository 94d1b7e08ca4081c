"""all2all bands, band emit (KMDB_HAS_ALL2ALL_BAND_EMIT): kmdb_all2all_rows_records[_device] emitting the block records of the band's block rows alone,
keyed relative to the band, on a state of its own per handle; kmdbh_band_streams; kmdb_all2all_rows_band_emit_stats_get; and the front-end's
`-band-path records` with KMDB_BAND_EMIT=1.

DEFINITION of the call: bit for bit what kmdb_all2all_rows_device writes — the cells [tri(row_lo), tri(row_hi)) of kmdb_all2all_dense_device.  Every
device check holds the band against the flat-form definition in numpy, against the tree band call and — where the triangle is small — against the slice
of the same handle's all2all_dense.  Every output buffer is a torch tensor filled with a sentinel with the band in its middle: 3 tri(N) words, or for the
collections of tens of thousands of samples the band with a margin either side; the words in front of the band and behind it must still hold the
sentinel after the call."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import all2all_rows_cases as RC
import all2all_rows_records_cases as RR
import band_emit_cases as BE
import variant_cases as VC
import wide_cases as W
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
HEADER = os.path.join(ROOT, "include", "kmdb_amd.h")
NEW_SYMBOLS = ("kmdb_all2all_rows_band_emit_stats_get", "kmdbh_band_streams")
SWITCHES = ("KMDB_K1N_MODE", "KMDB_ROW_MODE", "KMDB_BLOCK_WIDTH", "KMDB_SLICES", "KMDB_L2_MIN", "KMDB_L2", "KMDB_POOL_PERCENT", "KMDB_REC_PACKED",
            "KMDB_K1W_RUN", "KMDB_K1W_WAVES", "KMDB_NSEG", "KMDB_VERBOSE", "KMDB_BAND_EMIT", "KMDB_BAND_MAX_STREAMS")
# the three record paths of test_wide_conformance.py's MODES
MODES = {"few streams": {}, "rows, no L2": dict(KMDB_ROW_MODE=1, KMDB_L2=0), "rows, L2 from 11": dict(KMDB_ROW_MODE=1, KMDB_L2_MIN=11)}
FORM_NONE, FORM_WHOLE, FORM_BAND = 0, 1, 2
DENSE_WORDS = 1 << 24          # a triangle of up to that many cells is also taken whole (all2all_dense) and sliced
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
    assert re.search(r"^#define KMDB_HAS_ALL2ALL_BAND_EMIT 1$", src, re.M)
    assert re.search(r"^#define KMDB_ABI_VERSION 8$", src, re.M)
    for i, name in enumerate(("KMDB_BAND_EMIT_FORM_NONE", "KMDB_BAND_EMIT_FORM_WHOLE", "KMDB_BAND_EMIT_FORM_BAND")):
        assert re.search(r"^#define %s\s+%du\b" % (name, i), src, re.M), name
    assert (K.capi.BAND_EMIT_FORM_NONE, K.capi.BAND_EMIT_FORM_WHOLE, K.capi.BAND_EMIT_FORM_BAND) == (FORM_NONE, FORM_WHOLE, FORM_BAND)
    L = ctypes.CDLL(K.lib_path())
    for name in NEW_SYMBOLS:
        assert name in K.capi.EXPORTS and hasattr(L, name), name
        assert re.search(r"^int\s+%s\(" % name, src, re.M), name
    ctype = {"c_ulong": "uint64_t", "c_uint": "uint32_t", "c_double": "double"}
    for struct, fields in (("kmdb_all2all_rows_band_emit_stats", K.capi._All2allRowsBandEmitStats._fields_),
                           ("kmdb_band_geometry", K.capi._BandGeometry._fields_)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        decl = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|uint32_t|double)\s+([^;]+);", body) for n in names.split(",")]
        assert decl == [(ctype[t.__name__], f) for f, t in fields], struct
    for meth in ("all2all_rows_band_emit_stats", "band_streams"):
        assert hasattr(K.DeviceDB, meth), meth
    assert list(inspect.signature(K.band_streams).parameters) == ["n_samples", "width", "row_lo", "row_hi"]
    # the fields the statistics report
    names = [f for f, _ in K.capi._All2allRowsBandEmitStats._fields_]
    for f in ("form", "x_lo", "x_hi", "n_rows", "n_streams", "stream_base", "key_bits", "row_mode", "l2_on", "records", "est_records", "attempts",
              "state_bytes", "whole_state_bytes"):
        assert f in names, f


def test_null_arguments_are_refused_by_name(K):
    lib = K.capi.lib()
    assert lib.kmdb_all2all_rows_band_emit_stats_get(None, None) != 0
    assert b"kmdb_all2all_rows_band_emit_stats_get: null argument" in lib.kmdb_last_error()
    assert lib.kmdbh_band_streams(10, 32, 0, 5, None) != 0 and b"kmdbh_band_streams: null argument" in lib.kmdb_last_error()


@pytest.mark.parametrize("width", BE.GEOMETRY_WIDTHS)
def test_band_streams_against_the_closed_form(K, width):
    """kmdbh_band_streams (host only) against tri32(Xhi + 1) - tri32(Xlo) and its companions, for one-row bands at block edges, block-aligned bands,
    bands that cross an edge, [0, N) and empty bands"""
    seen = 0
    for N in BE.GEOMETRY_N:
        for lo, hi in BE.geometry_bands(width, N):
            got = K.band_streams(N, width, lo, hi)
            assert got == BE.geometry(width, lo, hi), (N, width, lo, hi, got)
            seen += 1
    assert seen > 100
    # the whole matrix is the case Xlo = 0, Xhi = NB - 1: every block pair
    for N in (4100, 92640, 92641):
        NB = -(-N // width)
        g = K.band_streams(N, width, 0, N)
        assert (g["x_lo"], g["x_hi"], g["n_rows"], g["n_streams"], g["stream_base"]) == (0, NB - 1, NB, NB * (NB + 1) // 2, 0), (N, g)
    # 92 640 samples at width 32 are the last the whole-matrix pipeline keys; 92 641 are beyond it
    if width == 32:
        assert K.band_streams(92640, 32, 0, 92640)["fits"] == 1 and K.band_streams(92641, 32, 0, 92641)["fits"] == 0


@pytest.mark.parametrize("width", BE.GEOMETRY_WIDTHS)
def test_band_streams_fits_flips_at_the_limit(K, width):
    N, lo, hi_fits, hi_beyond = BE.fits_flip(width)
    a, b = K.band_streams(N, width, lo, hi_fits), K.band_streams(N, width, lo, hi_beyond)
    assert a["n_streams"] + 1 < BE.STREAM_LIMIT <= b["n_streams"] + 1, (a, b)
    assert a["fits"] == 1 and b["fits"] == 0 and b["x_hi"] == a["x_hi"] + 1, (a, b)
    assert a == BE.geometry(width, lo, hi_fits) and b == BE.geometry(width, lo, hi_beyond)
    # the same band further up: relative keys — the base does not count
    up = K.band_streams(N, width, N - width, N)
    assert up["fits"] == 1 and up["n_rows"] == 1 and up["n_streams"] == up["x_hi"] + 1 and up["stream_base"] == BE.tri32(up["x_lo"]), up


def test_band_streams_refusals(K):
    for args, words in (((100, 31, 0, 5), "a block width of 31 lies outside 32 .. 64"), ((100, 65, 0, 5), "a block width of 65 lies outside 32 .. 64"),
                        ((100, 0, 0, 5), "a block width of 0 lies outside 32 .. 64"), ((100, 32, 9, 3), r"row_lo > row_hi \(9 > 3\)"),
                        ((100, 32, 3, 101), "row_hi 101 > the 100 samples")):
        with pytest.raises(K.KmdbError, match="kmdbh_band_streams: " + words):
            K.band_streams(*args)
    assert K.band_streams(100, 32, 100, 100) == BE.geometry(32, 100, 100)


def test_usage_text():
    usage = _cli().stderr
    assert "-band-path <tree|tiled|records>" in usage
    flat = " ".join(usage.split())
    for words in ("Beyond 2^22 block pairs", "records takes band emit by itself", "fewer than 2^22 streams per band", "KMDB_BAND_EMIT=1 | 0",
                  "form (whole emit | band emit)"):
        assert words in flat, words
    assert "up to about 185 000 samples (2^22 block pairs), KMDB_K1N_MODE=1 is refused" not in flat


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
    """set(name=value, ...) replaces ALL of the engine's switches by the ones given (None: unset); they are read when a handle or its band state is made"""
    def set_(**kw):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in kw.items():
            assert name in SWITCHES, name
            if value is not None:
                monkeypatch.setenv(name, str(value))
    set_()
    return set_


def _upload(K, S, pat, N, dev):
    _, view = VC.make_view(K, S, pat, N)
    return K.DeviceDB(view, device=dev)


def emit_band(d, N, lo, hi, dev, flags=0):
    """one call of kmdb_all2all_rows_records_device into the middle of a sentinel buffer — 3 tri(N) words with the band at tri(N), or (a triangle beyond
    DENSE_WORDS) the band with a margin of its own size, 4096 words at least, either side; the band, the call's stats and its band-emit stats"""
    import torch
    cells = tri(hi) - tri(lo)
    T = max(tri(N), 1) if tri(N) <= DENSE_WORDS else max(cells, 4096)
    sent = RR.SENTINEL - (1 << 32)
    buf = torch.full((2 * T + max(cells, T),), sent, dtype=torch.int32, device=torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    d.all2all_rows_records_device(buf.data_ptr() + 4 * T, lo, hi, flags=flags)
    torch.cuda.synchronize(dev)
    assert bool((buf[:T] == sent).all()), "band [%d, %d): words in front of the band were written" % (lo, hi)
    assert bool((buf[T + cells:] == sent).all()), "band [%d, %d): words behind the band were written" % (lo, hi)
    got = buf[T: T + cells].cpu().numpy().view(np.uint32)
    st = d.all2all_rows_records_stats()
    assert st["band_cells"] == cells, (lo, hi, st)
    return got, st, d.all2all_rows_band_emit_stats()


def check_emit(d, N, lo, hi, exp, dev, dense=None, tree=True, flags=0, form=FORM_BAND):
    """the band against the definition, against kmdb_all2all_rows (through its host variant) and against the slice of the handle's whole matrix; the
    form the call took and its geometry against the closed form"""
    got, st, be = emit_band(d, N, lo, hi, dev, flags)
    assert got.size == exp.size and np.array_equal(got, exp), "band [%d, %d): %d of %d cells differ from the definition" % (lo, hi, int((got != exp).sum()), exp.size)
    if tree:
        assert np.array_equal(got, d.all2all_rows(lo, hi)), "band [%d, %d) differs from kmdb_all2all_rows" % (lo, hi)
    if dense is not None:
        assert np.array_equal(got, dense[tri(lo): tri(hi)]), "band [%d, %d) differs from the slice of all2all_dense" % (lo, hi)
    if exp.size:
        assert st["path"] == 1 and be["form"] == form, (lo, hi, st, be)
        g = BE.geometry(st["width"], lo, hi)
        assert {k: be[k] for k in ("x_lo", "x_hi", "n_rows", "n_streams", "stream_base")} == {k: g[k] for k in ("x_lo", "x_hi", "n_rows", "n_streams", "stream_base")}, (lo, hi, be, g)
        assert (st["x_lo"], st["x_hi"]) == (g["x_lo"], g["x_hi"]) and st["units_run"] <= st["units_total"] and st["kernel_ms"] > 0, (lo, hi, st)
        if form == FORM_BAND:
            assert be["state_bytes"] > 0 and be["attempts"] >= 1 and (1 << be["key_bits"]) > be["n_streams"] + 1, be
            assert st["records"] == be["records"], (st, be)
    return got, st, be


def _dense(K, d, N):
    if tri(N) > DENSE_WORDS:
        return None
    full = d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK)
    full.setflags(write=False)
    return full


def _partition(d, N, full, dev, dense, seeds=range(2)):
    for seed in seeds:
        cuts = RC.seeded_cuts(N, 2000 + seed, 3 + 2 * seed)
        parts = [check_emit(d, N, a, b, full[tri(a): tri(b)], dev, dense)[0] for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts), full), cuts


def edge_one_row_bands(width, N):
    """every one-row band around `width` and around 2 width: the rows width - 1 .. width + 1 and 2 width - 1 .. 2 width + 1"""
    return [(r, r + 1) for r in list(range(width - 1, width + 2)) + list(range(2 * width - 1, 2 * width + 2)) if r < N]


@pytest.mark.gpu
@pytest.mark.parametrize("k1n", [0, 2])
@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("width", VC.WIDTHS)
def test_edge_forests(K, S, dev, env, width, rows, k1n):
    """variant_cases.edge_forest at both edge sizes under KMDB_ROW_MODE x KMDB_K1N_MODE, with KMDB_NSEG default and 64: a seeded partition into bands,
    every one-row band around width and 2 width, and [0, N)"""
    for N in VC.edge_sizes(width):
        pat, full = RR.edge_case(width, N)
        _, view = VC.make_view(K, S, pat, N)
        for nseg in (None, 64):
            env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=width, KMDB_ROW_MODE=rows, KMDB_K1N_MODE=k1n, KMDB_NSEG=nseg)
            d = K.DeviceDB(view, device=dev)
            dense = _dense(K, d, N)
            assert np.array_equal(dense, full)
            _partition(d, N, full, dev, dense, seeds=range(1 if nseg else 2))
            for lo, hi in edge_one_row_bands(width, N):
                _, st, be = check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev, dense)
                assert st["width"] == width and be["row_mode"] == rows and be["n_rows"] == 1, (st, be)
            _, st, be = check_emit(d, N, 0, N, full, dev, dense)
            # under band emit nothing is left to cull: every unit the call meets lies in the band
            assert st["units_run"] == st["units_total"] > 0 and be["n_streams"] == BE.tri32(-(-N // width)), (st, be)
            d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k1n", [0, 2])
@pytest.mark.parametrize("rows", [0, 1])
def test_light_forest(K, S, dev, env, rows, k1n):
    """variant_cases.light_forest: diagonal tiles that get first-block records of the matrix-core step only"""
    width, N = 50, 4 * 50 - 1
    pat = VC.light_forest(width, N)
    full = VC.definition(pat, N)
    env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=width, KMDB_ROW_MODE=rows, KMDB_K1N_MODE=k1n)
    d = _upload(K, S, pat, N, dev)
    dense = _dense(K, d, N)
    _partition(d, N, full, dev, dense)
    for lo, hi in RR.block_bands(width, N) + RR.one_row_bands(width, N)[::7]:
        check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev, dense)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_wide_forest(K, dev, env, mode):
    """wide_cases.wide_forest (width 32; heavy nodes of 11 blocks and more, lists of up to 36 blocks) under few streams / rows without the second level /
    rows with it from 11 blocks: one block row, two, a row range inside one block, all of it"""
    c = W.case("wide", 32, False)
    N, full = c["N"], c["exp"]
    _, view = VC.make_view(K, importlib.import_module("kmerdb_amd.synth"), c["pat"], N)
    env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=32, **MODES[mode])
    d = K.DeviceDB(view, device=dev)
    dense = _dense(K, d, N)
    for lo, hi in RR.block_bands(32, N) + [(N - 1, N), (31, 33), (20 * 32, 22 * 32)]:
        _, st, be = check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev, dense)
        assert be["row_mode"] == (0 if mode == "few streams" else 1) and be["l2_on"] == (1 if mode == "rows, L2 from 11" else 0), (mode, be)
        if mode == "rows, L2 from 11":
            assert st["tiles_run"] == st["tiles_total"] and ((lo, hi) != (0, N) or st["tiles_total"] > 0), st          # the band's tiles only are launched
        else:
            assert st["tiles_total"] == 0, (mode, st)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [63, 64, 65, 130])
def test_chain_forest(K, S, dev, env, depth):
    pat, N = RC.chain_forest(depth, True)
    full = VC.definition(pat, N)
    env(KMDB_BAND_EMIT=1)
    d = _upload(K, S, pat, N, dev)
    dense = _dense(K, d, N)
    for lo, hi in ((0, N), (N - 1, N), (depth // 2, depth // 2 + 3), (31, 33), (63, min(65, N))):
        if lo < hi:
            check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev, dense)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("l", [1024, 1025, 4100])
def test_long_list_forest(K, S, dev, env, l):
    pat, N = RC.long_list_forest(l)
    full = VC.definition(pat, N)
    env(KMDB_BAND_EMIT=1)
    d = _upload(K, S, pat, N, dev)
    dense = _dense(K, d, N)
    for lo, hi in ((N - 2, N), (0, 12), (N // 2, N // 2 + 70), (0, N) if l < 4100 else (N - 300, N - 100)):
        check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev, dense)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [None, 0])
def test_weight_forest(K, S, dev, env, packed):
    """all2all_rows_cases.weight_forest: weights around 2^31 and 2^32 whose sums wrap; and the edge forest's weights either side of 127 | 128 are in
    test_edge_forests"""
    pat, N = RC.weight_forest()
    full = VC.definition(pat, N)
    env(KMDB_BAND_EMIT=1, KMDB_REC_PACKED=packed)
    d = _upload(K, S, pat, N, dev)
    dense = _dense(K, d, N)
    for lo, hi in ((0, N), (5, 8), (7, 8), (1, 2)):
        check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev, dense)
    d.close()


@pytest.mark.gpu
def test_wide_code_forest(K, S, dev, env):
    """70 002 samples, the last two rows"""
    pat, N = RC.wide_code_forest()
    env(KMDB_BAND_EMIT=1)
    d = _upload(K, S, pat, N, dev)
    lo, hi = N - 2, N
    _, st, be = check_emit(d, N, lo, hi, RC.band_definition(pat, N, lo, hi), dev)
    assert be["n_rows"] == 1 and be["n_streams"] == be["x_hi"] + 1, be
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", [dict(KMDB_SLICES=3), dict(KMDB_POOL_PERCENT=1), dict(KMDB_REC_PACKED=0), dict(KMDB_K1W_WAVES=1)], ids=lambda s: "-".join(s))
def test_switches(K, S, dev, env, switch):
    """the edge forest at width 32 under KMDB_SLICES=3, KMDB_POOL_PERCENT=1, KMDB_REC_PACKED=0 and KMDB_K1W_WAVES=1: every band right (that the pools of
    KMDB_POOL_PERCENT=1 make the call repeat is test_small_pools_repeat's)"""
    width = 32
    N = VC.edge_sizes(width)[1]
    pat, full = RR.edge_case(width, N)
    env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=width, **switch)
    d = _upload(K, S, pat, N, dev)
    for lo, hi in RR.block_bands(width, N) + [(31, 33)]:
        _, st, be = check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
        if "KMDB_SLICES" in switch:
            assert st["slices"] == 3, st
    d.close()


@pytest.mark.gpu
def test_small_pools_repeat(K, S, dev, env):
    """KMDB_POOL_PERCENT=1 on the edge forest at width 32, many-streams path: the band state's sorted arrays are sized for the band's records — at one
    percent a chunk of 64 slots for the few hundred records of a block row — so the sort runs over, the arrays are doubled and the call repeated from a
    band zeroed again (the band's bytes only: emit_band checks the sentinel words around it); the band comes out right after the repeat, attempts > 1.
    (The few-streams path cannot be made to repeat by a band of this forest: its records arrive in a pool handed out through 256 sub-pools of one grab
    each, 65 536 slots at the least, which no percentage moves; test_switches holds its bands right under the switch.)"""
    width = 32
    N = VC.edge_sizes(width)[1]
    pat, full = RR.edge_case(width, N)
    env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=width, KMDB_POOL_PERCENT=1, KMDB_ROW_MODE=1)
    d = _upload(K, S, pat, N, dev)
    lo, hi = RR.block_bands(width, N)[0]
    _, st, be = check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
    print("KMDB_POOL_PERCENT=1: attempts", be["attempts"], "records", be["records"], "estimate", be["est_records"], "state bytes", be["state_bytes"])
    assert be["attempts"] > 1 and be["row_mode"] == 1 and st["sized_call"] == 1, (st, be)
    for lo, hi in RR.block_bands(width, N)[1:] + [(31, 33)]:
        check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("k1n", [0, 2])
def test_partition_identity(K, dev, env, k1n, mode):
    """a partition of [0, N) at block-row boundaries: every record of the whole call is emitted by exactly one band — the bands' records sum to
    kmdb_stats.n_records of a whole call on an identically made handle, and no band emits more than the whole call"""
    c = W.case("wide", 32, False)
    N, full = c["N"], c["exp"]
    _, view = VC.make_view(K, importlib.import_module("kmerdb_amd.synth"), c["pat"], N)
    # (rows 0 | rows 1 with the second level off | on: the second level exists in row mode only)
    sw = dict(KMDB_BLOCK_WIDTH=32, KMDB_K1N_MODE=k1n, **MODES[mode])
    env(**sw)
    whole = K.DeviceDB(view, device=dev)
    assert np.array_equal(whole.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), full)
    n_records = whole.stats()["n_records"]
    whole.close()
    env(KMDB_BAND_EMIT=1, **sw)
    d = K.DeviceDB(view, device=dev)
    cuts = [0, 32, 5 * 32, 6 * 32, 20 * 32, 35 * 32, N]
    total = 0
    for lo, hi in zip(cuts, cuts[1:]):
        _, st, be = check_emit(d, N, lo, hi, full[tri(lo): tri(hi)], dev, tree=False)
        assert be["records"] <= n_records, (lo, hi, be, n_records)
        total += be["records"]
    assert total == n_records > 0, (total, n_records)
    d.close()


COUNTS = ("path", "width", "n_records", "n_direct", "n_wide", "n_chunks", "n_joined")


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [0, 1])
def test_one_handle(K, S, dev, env, rows):
    """whole call, band-emit call, whole call on one handle: both matrices equal, kmdb_stats of the whole calls equal, state_bytes > 0; a second band with
    more streams than the first makes the state anew and is right.  Held equal between the two whole calls: path, width, n_records, n_direct, n_wide,
    n_chunks, n_joined (COUNTS) — what the call did.  Not held equal: the times (kernel_ms, k0_ms ... k2_ms, upload_ms: measurements), sized_call (the
    first call of a handle measures its launch sizes, the later one must not: asserted 0) and device_bytes, which counts what is resident and so grows
    by the band state (asserted: at least the first call's plus state_bytes)"""
    width, N = 50, 4 * 50 - 1
    pat, full = RR.edge_case(width, N)
    env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=width, KMDB_ROW_MODE=rows)
    d = _upload(K, S, pat, N, dev)
    NF = K.capi.FLAG_NO_FALLBACK
    m1 = d.all2all_dense(flags=NF)
    s1 = d.stats()
    assert d.all2all_rows_band_emit_stats()["state_bytes"] == 0
    _, st, b1 = check_emit(d, N, 10, 40, full[tri(10): tri(40)], dev, tree=False, flags=NF)
    assert b1["state_bytes"] > 0 and b1["whole_state_bytes"] > 0 and b1["n_streams"] == 1, b1
    m2 = d.all2all_dense(flags=NF)
    s2 = d.stats()
    assert np.array_equal(m1, full) and np.array_equal(m2, full)
    assert {k: s1[k] for k in COUNTS} == {k: s2[k] for k in COUNTS} and s2["sized_call"] == 0, (s1, s2)
    assert s2["device_bytes"] >= s1["device_bytes"] + b1["state_bytes"], (s1, s2, b1)
    _, st, b2 = check_emit(d, N, 120, N, full[tri(120):], dev, flags=NF)
    assert b2["n_streams"] > b1["n_streams"] and b2["n_rows"] == 2 and b2["state_bytes"] > 0, (b1, b2)
    _, st, b3 = check_emit(d, N, 10, 40, full[tri(10): tri(40)], dev, flags=NF)          # the first band again, inside the larger state
    assert b3["records"] == b1["records"] and b3["state_bytes"] >= b2["state_bytes"], (b1, b2, b3)
    assert np.array_equal(d.all2all_dense(flags=NF), full)
    d.close()


@pytest.mark.gpu
def test_band_emit_0_is_the_parent_form(K, S, dev, env):
    """KMDB_BAND_EMIT=0 and unset: the same band, equal, form == whole emit, records == the whole call's; no band state is made"""
    width, N = 50, 4 * 50 - 1
    pat, full = RR.edge_case(width, N)
    for value in (0, None):
        env(KMDB_BAND_EMIT=value, KMDB_BLOCK_WIDTH=width)
        d = _upload(K, S, pat, N, dev)
        _, st, be = check_emit(d, N, 60, 130, full[tri(60): tri(130)], dev, form=FORM_WHOLE)
        assert be["state_bytes"] == 0 and be["whole_state_bytes"] > 0 and be["n_streams"] == BE.geometry(width, 60, 130)["n_streams"], be
        assert np.array_equal(d.all2all_dense(flags=K.capi.FLAG_NO_FALLBACK), full) and d.stats()["n_records"] == st["records"] == be["records"], (st, be)
        d.close()


@pytest.mark.gpu
def test_band_max_streams(K, S, dev, env):
    """KMDB_BAND_MAX_STREAMS=1000 on the edge forest at width 32 over 46 blocks (tri32(46) = 1081 streams; the sizes of the other tests have 10).  A band
    over the cap takes the tree call: path 2, the same cells as the slice of the handle's whole matrix; with KMDB_FLAG_NO_FALLBACK it fails naming the
    streams and leaves the buffer untouched.  A band under the cap runs: the last block row, 46 streams, against the definition of its rows too"""
    import torch
    width, N = 32, 46 * 32 - 1
    pat = VC.edge_forest(width, N)
    env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=width, KMDB_BAND_MAX_STREAMS=1000)
    d = _upload(K, S, pat, N, dev)
    dense = _dense(K, d, N)
    got, st, be = emit_band(d, N, 0, N, dev)
    assert np.array_equal(got, dense) and st["path"] == 2 and be["form"] == FORM_NONE and be["n_streams"] == 1081, (st, be)
    lo = 2 * width + 5                                              # block rows 2 .. 45: 1078 streams
    got, st, be = emit_band(d, N, lo, N, dev)
    assert np.array_equal(got, dense[tri(lo):]) and st["path"] == 2 and be["n_streams"] == 1078, (st, be)
    t = torch.full((tri(N),), 77, dtype=torch.int32, device=torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    with pytest.raises(K.KmdbError, match=r"kmdb_all2all_rows_records_device: band emit unavailable: the band's 1081 streams \(block rows 0 to 45 of width 32\) reach the limit of 1000 streams"):
        d.all2all_rows_records_device(t.data_ptr(), 0, N, flags=K.capi.FLAG_NO_FALLBACK)
    torch.cuda.synchronize(dev)
    assert bool((t == 77).all()), "a refused call wrote into the caller's buffer"
    lo = 45 * width
    _, st, be = check_emit(d, N, lo, N, RC.band_definition(pat, N, lo, N), dev, dense, flags=K.capi.FLAG_NO_FALLBACK)
    assert be["n_streams"] == 46 and st["path"] == 1, (st, be)
    # block rows 14 .. 45: 976 streams, under the cap as well — 32 block rows in one band
    _, st, be = check_emit(d, N, 14 * width, N, dense[tri(14 * width):].copy(), dev, dense, tree=False)
    assert be["n_streams"] == 976 and be["n_rows"] == 32, be
    d.close()


@pytest.mark.gpu
def test_band_max_streams_0_or_no_number_is_ignored(K, S, dev, env):
    """KMDB_BAND_MAX_STREAMS=0, or a value that is no number, does not send every band to the tree call: the limit stays 2^22"""
    width = 32
    N = VC.edge_sizes(width)[1]
    pat, full = RR.edge_case(width, N)
    for value in ("0", "many"):
        env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=width, KMDB_BAND_MAX_STREAMS=value)
        d = _upload(K, S, pat, N, dev)
        check_emit(d, N, 0, N, full, dev, flags=K.capi.FLAG_NO_FALLBACK)
        d.close()


@pytest.mark.gpu
def test_k1n_mode_1_is_refused_by_name(K, S, dev, env):
    import torch
    width = 32
    N = VC.edge_sizes(width)[1]
    pat, full = RR.edge_case(width, N)
    env(KMDB_BAND_EMIT=1, KMDB_BLOCK_WIDTH=width, KMDB_K1N_MODE=1)
    d = _upload(K, S, pat, N, dev)
    t = torch.full((tri(9) - tri(3),), 77, dtype=torch.int32, device=torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_records_device: this handle was made under KMDB_K1N_MODE=1"):
        d.all2all_rows_records_device(t.data_ptr(), 3, 9)
    with pytest.raises(K.KmdbError, match="kmdb_all2all_rows_records: this handle was made under KMDB_K1N_MODE=1"):
        d.all2all_rows_records(3, 9)
    torch.cuda.synchronize(dev)
    assert bool((t == 77).all()), "a refused call wrote into the caller's buffer"
    assert np.array_equal(d.all2all_dense(), full)
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, beyond 2^22 block pairs: KMDB_BAND_EMIT unset
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_expected():
    pat, N = BE.far_forest()
    return {(lo, hi): RC.band_definition(pat, N, lo, hi) for lo, hi in BE.FAR_BANDS}


@pytest.mark.gpu
@pytest.mark.parametrize("k1n", [0, 2])
@pytest.mark.parametrize("rows", [0, 1])
def test_beyond_the_limit(K, S, dev, env, far_expected, rows, k1n):
    """band_emit_cases.far_forest: 100 000 samples at width 32 are 4.88 M block pairs — the whole-matrix pipeline refuses them ("too many block pairs"),
    and without band emit kmdb_all2all_rows_records with KMDB_FLAG_NO_FALLBACK fails with that reason.  With KMDB_BAND_EMIT unset the records band call
    takes band emit by itself: every band equals its definition and kmdb_all2all_rows, path == 1, form == band emit; the whole-matrix call on the
    same handle still reports its reason"""
    pat, N = BE.far_forest()
    env(KMDB_BLOCK_WIDTH=BE.FAR_WIDTH, KMDB_ROW_MODE=rows, KMDB_K1N_MODE=k1n)
    d = _upload(K, S, pat, N, dev)
    NF = K.capi.FLAG_NO_FALLBACK
    for lo, hi in BE.FAR_BANDS:
        exp = far_expected[(lo, hi)]
        assert exp.any(), (lo, hi)
        _, st, be = check_emit(d, N, lo, hi, exp, dev, flags=NF)
        # (KMDB_ROW_MODE=0 is followed as far as the one-pass sort's LDS holds the band's streams: the 9 372 of the last 70 rows fit it, the 12 494 of the
        # last 100 do not and take the many-streams path)
        assert st["width"] == BE.FAR_WIDTH and be["whole_state_bytes"] == 0, (st, be)
        assert be["row_mode"] == BE.expected_row_mode(be["n_streams"], rows, BE.FAR_WIDTH), (lo, hi, rows, be)
        if (lo, hi) == (N - 100, N):
            assert be["n_streams"] == 12494 and be["row_mode"] == 1, be
            # the same band again: the state made for it is kept (a state made anew measures its launch sizes again)
            got2, st2, be2 = emit_band(d, N, lo, hi, dev, flags=NF)
            assert np.array_equal(got2, exp) and st2["sized_call"] == 0 and be2["state_bytes"] == be["state_bytes"] and be2["row_mode"] == 1, (st2, be2)
        if (lo, hi) == (N - 70, N):
            assert be["n_streams"] == 9372 and be["row_mode"] == rows, be
        assert be["stream_base"] == BE.tri32(lo // 32) and be["n_streams"] + 1 < BE.STREAM_LIMIT, be
    assert d.fallback_reason() == "too many block pairs"
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, composed: the banded sparse call and the front-end
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def virus_emit(K, dev, golden_dir):
    """(HostDB, DeviceDB made under KMDB_BAND_EMIT=1) of virus_k18.db, and kmdb_all2all_sparse_filtered's rows without and with bounds"""
    old = os.environ.get("KMDB_BAND_EMIT")
    os.environ["KMDB_BAND_EMIT"] = "1"
    try:
        h = K.HostDB(os.path.join(golden_dir, "virus_k18.db"))
        d = K.DeviceDB(h, device=dev)
        similar = d.all2all_sparse_filtered([("jaccard", 0.5, None)], h.sample_kmers)
        cap = int(np.median(similar.val))
        forms = {"plain": ([], None), "bounds": ([("jaccard", 0.5, None), ("num-kmers", None, cap)], None), "measure": ([], "mash")}
        wants = {k: (f, m, d.all2all_sparse_filtered(f, h.sample_kmers, measure=m)) for k, (f, m) in forms.items()}
        d.all2all_rows_records(3, 9)                             # (KMDB_BAND_EMIT is read at the handle's first records band call)
        assert d.all2all_rows_band_emit_stats()["form"] == FORM_BAND
    finally:
        if old is None:
            del os.environ["KMDB_BAND_EMIT"]
        else:
            os.environ["KMDB_BAND_EMIT"] = old
    yield h, d, wants
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 7, 64, 165, 170])
def test_banded_sparse_call(K, virus_emit, R):
    h, d, wants = virus_emit
    N = h.N
    for form, (filters, measure, want) in wants.items():
        assert want.nnz > 0 and (form != "bounds" or want.nnz < wants["plain"][2].nnz), form
        got = d.all2all_sparse_filtered_banded(R, filters, h.sample_kmers, measure=measure, path="records")
        assert got.n_rows == want.n_rows and got.nnz == want.nnz
        assert np.array_equal(got.row_ptr, want.row_ptr) and np.array_equal(got.col, want.col) and np.array_equal(got.val, want.val)
        assert (got.measure is None) == (want.measure is None) and (want.measure is None or np.array_equal(got.measure, want.measure))
        be, rs = d.all2all_rows_band_emit_stats(), d.all2all_banded_records_stats()
        assert be["form"] == FORM_BAND and rs["bands"] == -(-N // R), (be, rs)


def _lines(path):
    return _read(path).splitlines(keepends=True)


@pytest.fixture()
def fe(dev, golden_dir, tmp_path):
    return (lambda n: os.path.join(golden_dir, n)), (lambda n: str(tmp_path / n))


REC = ("-band-path", "records")
EMIT = {"KMDB_BAND_EMIT": "1"}


@pytest.mark.gpu
def test_front_end_dense(fe):
    g, t = fe
    db = g("virus_k18.db")
    want = _lines(g("virus.k18.csv"))
    r = _cli("all2all", "-band-rows", "40", *REC, db, t("b.csv"), env=dict(EMIT, KMDB_VERBOSE="1"))
    assert _read(t("b.csv")) == _read(g("virus.k18.csv"))
    assert r.stderr.count("[kmdb] all2all rows records: rows ") == 5 and r.stderr.count(", form band emit, ") == 5, r.stderr
    m = re.search(r"rows 120 to 160, .* form band emit, (\d+) streams from (\d+) in (\d+) key bits, (\d+) attempts, band state (\d+) bytes", r.stderr)
    assert m and int(m.group(5)) > 0, r.stderr
    r = _cli("all2all", "-rows", "100:165", *REC, db, t("a.csv"), env=dict(EMIT, KMDB_VERBOSE="1"))
    assert _lines(t("a.csv")) == want[:2] + want[102:167] and ", form band emit, " in r.stderr
    # without the switch the same command names the parent form
    r = _cli("all2all", "-rows", "100:165", *REC, db, t("a0.csv"), env={"KMDB_VERBOSE": "1"})
    assert _read(t("a0.csv")) == _read(t("a.csv")) and ", form whole emit, " in r.stderr


@pytest.mark.gpu
def test_front_end_sparse(fe):
    g, t = fe
    db = g("virus_k18.db")
    want = _lines(g("virus.k18.sparse.csv"))
    _cli("all2all-sp", "-band-rows", "40", *REC, db, t("b.csv"), env=EMIT)
    assert _read(t("b.csv")) == _read(g("virus.k18.sparse.csv"))
    _cli("all2all", "-sparse", "-rows", "100:165", *REC, db, t("a.csv"), env=EMIT)
    assert _lines(t("a.csv")) == want[:2] + want[102:167]
    sw = ("-min", "jaccard:0.5", "-max", "num-kmers:20000")
    _cli("all2all-sp", *sw, "-band-rows", "40", db, t("f.want"))
    _cli("all2all-sp", *sw, "-band-rows", "40", *REC, db, t("f.csv"), env=EMIT)
    assert _read(t("f.csv")) == _read(t("f.want")) and len(_read(t("f.csv"))) > 100
    _cli("all2all-sp", *sw, "-rows", "100:165", db, t("g.want"))
    _cli("all2all-sp", *sw, "-rows", "100:165", *REC, db, t("g.csv"), env=EMIT)
    assert _read(t("g.csv")) == _read(t("g.want"))


@pytest.mark.gpu
def test_front_end_distance(fe):
    g, t = fe
    db = g("virus_k18.db")
    want = _lines(g("virus.k18.csv.jaccard"))
    _cli("all2all", "-distance", "jaccard", "-band-rows", "40", *REC, db, t("k.csv"), env=EMIT)
    assert _read(t("k.csv")) == _read(g("virus.k18.csv.jaccard"))
    _cli("all2all", "-distance", "jaccard", "-rows", "100:165", *REC, db, t("j.csv"), env=EMIT)
    assert _lines(t("j.csv")) == want[:1] + want[101:166]
    sw = ("-distance", "ani", "-distance", "min", "-min", "0.5")
    _cli("all2all-sp", *sw, "-rows", "100:165", "-band-rows", "40", db, t("two.want"))
    _cli("all2all-sp", *sw, "-rows", "100:165", "-band-rows", "40", *REC, db, t("two.got"), env=EMIT)
    for suffix in (".ani", ".min"):
        assert len(_lines(t("two.want" + suffix))) == 66 and _read(t("two.got" + suffix)) == _read(t("two.want" + suffix)), suffix
