"""The distance mode on the device (kmdb_distance_*, csrc/distance.hip) against the row rules restated in tests/distance_cases.py and the
reference's goldens: byte-equal text for every grammar quirk of the host loop, every measure and output form, the shapes at which the
classification and the scans can go wrong, the cells left to the host, and the input the device path declines."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distance_cases as DC
from conftest import ROOT
from test_host_cpu import DISTANCE_CASES

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
MODES = {  # name -> (flags of the device handle, state the restated loop starts in)
    "dense": ({}, {}),
    "triangle": ({"triangle": True}, {"triangle": True}),
    "sparse-out": ({"sparse_out": True}, {"sparse_out": True}),
    "sparse-in": ({"sparse_in": True}, {"sparse_out": True}),
    "phylip": ({"phylip": True}, {"phylip": True}),
    "phylip-triangle": ({"phylip": True, "triangle": True}, {"phylip": True, "triangle": True}),
}


@pytest.fixture(scope="module")
def L(K):
    lib = K.capi.lib()
    lib.kmdbh_metric.restype = ctypes.c_double
    return lib


def both(K, L, text, mode, measure, k, counts, bounds=(), first_row=0, cache=None):
    """-> (the device's text, the restated loop's text, the handle's stats)"""
    flags, state = MODES[mode]
    kmer = [b for b in bounds if b[0] == "num-kmers"]
    other = [b for b in bounds if b[0] != "num-kmers"]
    r = DC.Rules(L, measure, k, counts, bounds=other, kmer_lo=int(kmer[0][1]) if kmer and kmer[0][1] is not None else 0,
                 kmer_hi=int(kmer[0][2]) if kmer and kmer[0][2] is not None else DC.M32, cache=cache, **state)
    want = r.rows(text, first_row)
    d = K.Distance(measure, k, counts, filters=list(bounds), **flags)
    got, status = d.rows(text, first_row)
    assert status == 0, getattr(d, "declined", "")
    st = d.stats()
    d.close()
    return got, want, st


def run_cli(tmp_path, data, opts, env_extra=None):
    src, out = tmp_path / "table", tmp_path / "out"
    src.write_bytes(data)
    env = dict(os.environ, KMDB_DISTANCE_DEVICE="1", KMDB_VERBOSE="1", **(env_extra or {}))
    r = subprocess.run([EXE, "distance"] + list(opts) + [str(src), str(out)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return out.read_bytes(), r.stderr


def cli_stats(stderr):
    """-> [rows, cells read, cells written, host cells, calls], summed over the handles the front-end used"""
    rows = re.findall(r"distance on the device: calls (\d+), rows (\d+), cells read (\d+), cells written (\d+), host cells (\d+)", stderr)
    assert rows, stderr
    return [sum(int(r[i]) for r in rows) for i in (1, 2, 3, 4, 0)]


# ---- 1. the reference's goldens through the command line -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DISTANCE_CASES, ids=lambda c: c[2] + ":" + "_".join(c[0]))
def test_goldens_on_the_device(golden_dir, tmp_path, case):
    opts, src, want = case
    got, err = run_cli(tmp_path, open(os.path.join(golden_dir, src), "rb").read(), opts)
    assert got == open(os.path.join(golden_dir, want), "rb").read()
    assert "declined" not in err, err
    rows, read, written, host, calls = cli_stats(err)
    assert rows > 0 and written > 0 and host < written, err       # the device wrote the cells


# ---- 2. grammar quirks ---------------------------------------------------------------------------------------------------------------------
COUNTS4 = [1000, 2000, 3000, 4000]
DENSE_QUIRKS = {
    "row-0-empty": b"s0,1000,\ns1,2000,17,\ns2,3000,5,9,\n",
    "last-line-without-newline": b"s0,1000,1,2,3,4,\ns1,2000,5,6,7,8,",
    "final-field-of-one-character-dropped": b"s0,1000,11,22,33,4\ns1,2000,1,2,3,\n",
    "final-field-of-two-characters-read": b"s0,1000,11,22,33,44\ns1,2000,1,2,3,44",
    "more-cells-than-n": b"s0,1000,1,2,3,4,5,6,7,\ns1,2000,8,9,10,11,12,\n",
    "fewer-cells-than-n": b"s0,1000,1,\ns1,2000,\ns2,3000,7,8,\n",
    "empty-cells": b"s0,1000,,5,,\ns1,2000,,,\ns2,3000,,\n",
    "ten-digit-counts": b"s0,4294967295,4294967295,1000000000,0000000007,9,\ns1,4000000000,3999999999,1,2,3,\n",
    "counts-that-wrap": b"s0,4294967297,4294967296,9999999999,8589934593,4294967306,\ns1,9999999999,9999999999,8589934592,1,2,\n",
    "a-plus-b-minus-c-wraps": b"s0,10,5000,1011,3011,4011,\ns1,0,1001,2001,3001,4001,\n",
    "names": "s 0 with blanks,1000,1,2,3,4,\ns:1:colons,2000,5,6,7,8,\nźłość-üñí,3000,9,10,11,12,\n,4000,1,1,1,1,\n".encode(),
}
SPARSE_QUIRKS = {
    "columns-0-and-n-plus-1-and-count-0": b"s0,1000,0:5,1:6,5:7,4:8,2:0,\ns1,2000,4294967297:3,3:9,\n",
    "last-line-without-newline": b"s0,1000,1:6,4:8,\ns1,2000,2:7,3:9",
    "final-pair-of-few-characters": b"s0,1000,1:6,4:\ns1,2000,2:7,3\ns2,3000,2:7,3:\ns3,4000,1:\n",
    "wrapping-counts": b"s0,4294967297,1:4294967296,2:9999999999,0000000003:8589934593,\ns1,10,1:5000,4:4011,\n",
    "empty-rows-and-names": "s 0,1000,\ns:1,2000,\nü,3000,2:5,\n".encode(),
}


@pytest.mark.parametrize("measure", ["jaccard", "mash", "cosine"])
@pytest.mark.parametrize("mode", ["dense", "triangle", "sparse-out", "phylip", "phylip-triangle"])
@pytest.mark.parametrize("name", sorted(DENSE_QUIRKS))
def test_dense_grammar_quirks(K, L, name, mode, measure):
    bounds = [(measure, None, None), ("num-kmers", 1, None)] if mode == "sparse-out" else []
    for first_row in (0, 2):
        got, want, st = both(K, L, DENSE_QUIRKS[name], mode, measure, 21, COUNTS4, bounds, first_row)
        assert got == want, (got, want)


@pytest.mark.parametrize("measure", ["jaccard", "ani", "num-kmers"])
@pytest.mark.parametrize("name", sorted(SPARSE_QUIRKS))
def test_sparse_grammar_quirks(K, L, name, measure):
    for bounds in ([], [("num-kmers", 6, 5000)]):
        got, want, st = both(K, L, SPARSE_QUIRKS[name], "sparse-in", measure, 21, COUNTS4, bounds)
        assert got == want, (got, want)


@pytest.mark.parametrize("measure", DC.METRICS)
def test_samples_without_kmers(K, L, measure):
    """a = b = 0: divisions by zero, NaN and infinities — the host's cells, written as the host writes them"""
    counts = [0, 7, 0]
    text = b"s0,0,0,0,0,\ns1,0,5,5,5,\ns2,7,0,7,3,\n"
    for mode in ("dense", "sparse-out", "phylip"):
        got, want, st = both(K, L, text, mode, measure, 18, counts)
        assert got == want, (mode, got, want)
    got, want, st = both(K, L, b"s0,0,1:5,3:2,\ns1,7,1:1,2:7,3:0,\n", "sparse-in", measure, 18, counts)
    assert got == want, (got, want)


def test_no_columns_and_no_rows(K, L):
    for mode in MODES:
        d = K.Distance("mash", 18, [], **MODES[mode][0])
        assert d.rows(b"") == (b"", 0)
        d.close()
        if mode != "sparse-in":
            got, want, st = both(K, L, b"s0,5,\ns1,6,1,2,\n", mode, "mash", 18, [])
            assert got == want


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------------------------
def wide_and_narrow(rng, n_wide, n_rows):
    counts = DC.random_counts(rng, n_wide)
    wide = b"wide,4000000," + b"".join(b"%d," % v for v in rng.integers(0, 3_000_000, n_wide)) + b"\n"
    narrow = b"".join(b"r%d,%d," % (i, 3_000_000 + i) + b"".join(b"%d," % v for v in rng.integers(1, 3_000_000, rng.integers(0, 4))) + b"\n"
                      for i in range(n_rows))
    return counts, wide, narrow


@pytest.mark.parametrize("mode", ["sparse-out", "phylip", "phylip-triangle"])
def test_one_wide_row_and_many_narrow_rows(K, L, mode):
    """a row longer than any workgroup's tile, thousands of rows of 0 - 3 cells, and both in one piece (either order)"""
    rng = np.random.default_rng(5)
    counts, wide, narrow = wide_and_narrow(rng, 5000, 3000)
    cache = {}
    for text in (wide, narrow, narrow + wide + narrow, wide + narrow):
        got, want, st = both(K, L, text, mode, "mash", 21, counts, first_row=1, cache=cache)
        assert got == want
        assert st["rows"] == text.count(b"\n") and st["cells_written"] > 0


def test_dense_rows_are_as_wide_as_the_table(K, L):
    """dense output: n (triangle: min(row, n)) values per row whatever the row holds"""
    rng = np.random.default_rng(6)
    counts, wide, narrow = wide_and_narrow(rng, 700, 90)
    for mode in ("dense", "triangle"):
        got, want, st = both(K, L, narrow + wide + narrow, mode, "ani", 21, counts, first_row=3)
        assert got == want


def triangle_table(rng, n, sparse):
    names = [b"smp%d" % i for i in range(n)]
    counts = DC.random_counts(rng, n)
    cells = rng.integers(1000, 3_000_000, (n, n)) * (rng.random((n, n)) >= 0.3)
    body = (DC.sparse_body if sparse else DC.dense_body)(names, counts, cells, triangle=True)
    return DC.header(20, names, counts) + body


@pytest.mark.parametrize("piece", ["4096", "1"])
@pytest.mark.parametrize("form", ["dense", "dense-sparse-out", "dense-phylip", "sparse", "sparse-sparse-out"])
def test_pieces_carry_the_row_number(L, tmp_path, piece, form):
    """a triangle of 300 samples cut into pieces of 4096 bytes and of one row: every row keeps its own min(row, n); a sparse triangle's
    row 0 holds no cells and is written as the dense row it is until the first pair is met"""
    rng = np.random.default_rng(8)
    data = triangle_table(rng, 300, form.startswith("sparse"))
    opts = {"dense": [], "dense-sparse-out": ["-sparse", "-min", "0.2"], "dense-phylip": ["-phylip-out"], "sparse": [], "sparse-sparse-out": ["-sparse"]}[form] + ["jaccard"]
    got, err = run_cli(tmp_path, data, opts, {"KMDB_DISTANCE_BYTES_PER_PIECE": piece})
    assert "declined" not in err, err
    assert got == DC.distance_file(L, data, opts)
    rows, read, written, host, calls = cli_stats(err)
    assert rows == 300 and host <= written
    # one row a call — row 0, which holds no cells, waits for the first row that has some: it travels with row 1, or, where the loop
    # writes it as a dense row in front of sparse ones, goes through a handle of its own; several rows a call
    assert calls == (300 if form == "sparse" else 299) if piece == "1" else 10 < calls < 299, calls


# ---- 4. every measure x every form ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table600(L):
    rng = np.random.default_rng(20240)
    counts = DC.random_counts(rng, 400)
    row_counts = DC.random_counts(rng, 600)
    cells = rng.integers(1000, 3_000_001, (600, 400)) * (rng.random((600, 400)) >= 0.3)
    names = [b"q%d" % i for i in range(600)]
    return {"counts": counts, "row_counts": row_counts, "cells": cells, "dense": DC.dense_body(names, row_counts, cells),
            "sparse": DC.sparse_body(names, row_counts, cells), "cache": {}}


@pytest.mark.parametrize("mode", ["dense", "triangle", "sparse-out", "sparse-in", "phylip"])
@pytest.mark.parametrize("measure", DC.METRICS)
def test_every_measure_and_form(K, L, table600, measure, mode):
    """600 x 400 cells, 30 % zeros; bounds on the measure — the lower one exactly a cell's host value — and on num-kmers.  The device decides
    all but a sliver: at margin 2^-20 the rounding-boundary share of this generator is below 1.2e-5 for every measure, and a bound on a
    cell's own value adds that cell (and its equals)."""
    t = table600
    m = DC.METRICS.index(measure)
    # the bound lies on the value of one cell of row 0: the one at the end of the row's range that keeps the other cells
    a0 = int(t["row_counts"][0])
    row0 = [L.kmdbh_metric(m, ctypes.c_uint32(int(c)), ctypes.c_uint32(a0), ctypes.c_uint32(int(b)), 19)
            for c, b in zip(t["cells"][0], t["counts"]) if 2000 < c < 2_900_000]
    falls = measure in ("mash", "mash-query")                   # distances fall as the counts rise: there the cell's value is the upper bound
    on_a_cell = max(row0) if falls else min(row0)
    far = on_a_cell + abs(on_a_cell) * 1e6 + 1
    bounds = [(measure, -1.0, on_a_cell) if falls else (measure, on_a_cell, far)]
    if measure != "num-kmers":
        bounds.append(("num-kmers", 2000, 2_900_000))
    got, want, st = both(K, L, t["sparse" if mode == "sparse-in" else "dense"], mode, measure, 19, t["counts"], bounds, first_row=5, cache=t["cache"])
    assert got == want
    assert st["cells_written"] > 10_000 and st["host_cells"] <= 1e-3 * st["cells_written"], st
    if mode in ("sparse-out", "sparse-in") and measure != "num-kmers":
        assert st["host_cells"] >= 1, st                        # the cell the bound lies on (a count is an integer: nothing to settle)


# ---- 5. boundary cells ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["jaccard", "min", "mash", "ani"])
@pytest.mark.parametrize("mode", ["dense", "sparse-out", "sparse-in", "phylip"])
def test_boundary_cells_are_the_hosts(K, L, mode, measure):
    """c = 1, a = 10^6, b = 10^6 + 1: jaccard is 5e-7, |v| * 1e6 + 0.5 is 1.0 to the last bit — the value the six decimals turn on"""
    counts = [1_000_001, 1_000_001, 1_000_001]
    if mode == "sparse-in":
        text = b"s0,1000000,1:1,2:3,3:1000000,\ns1,1000000,1:1000000,3:1,\n"
    else:
        text = b"s0,1000000,1,3,1000000,\ns1,1000000,1000000,0,1,\n"
    got, want, st = both(K, L, text, mode, measure, 20, counts)
    assert got == want, (got, want)
    if measure == "jaccard":
        assert st["host_cells"] >= 2, st                        # the two cells with c = 1
    # a bound on each crafted value: the bound's margin sends the cell to the host as well
    if mode in ("sparse-out", "sparse-in"):
        for c in (1, 3, 1_000_000):
            v = L.kmdbh_metric(DC.METRICS.index(measure), ctypes.c_uint32(c), ctypes.c_uint32(1_000_000), ctypes.c_uint32(1_000_001), 20)
            for bounds in ([(measure, v, None)], [(measure, None, v)], [(measure, np.nextafter(v, 9.0), None)], [(measure, None, np.nextafter(v, -9.0))]):
                got, want, st = both(K, L, text, mode, measure, 20, counts, bounds)
                assert got == want, (bounds, got, want)
                assert st["host_cells"] >= 1


# ---- 6. declined input ---------------------------------------------------------------------------------------------------------------------
DECLINED = [
    ("a-row-mixes-pairs-and-cells", {"sparse_in": True}, b"s0,5,1:2,3,\n", "plain cell"),
    ("a-row-mixes-cells-and-pairs", {}, b"s0,5,3,1:2,\n", "pair"),
    ("a-plain-cell-under-sparse-in", {"sparse_in": True}, b"s0,5,1:2,\ns1,6,7,\n", "plain cell"),
    ("a-pair-without-sparse-in", {"sparse_out": True}, b"s0,5,1,\ns1,6,2:7,\n", "pair"),
    ("eleven-digits", {}, b"s0,5,12345678901,\n", "10 digits"),
    ("eleven-digits-in-the-count", {}, b"s0,12345678901,1,\n", "10 digits"),
    ("a-sign", {}, b"s0,5,-3,\n", "neither a digit nor a separator"),
    ("a-blank", {}, b"s0,5, 3,\n", "neither a digit nor a separator"),
    ("a-carriage-return", {}, b"s0,5,3,\r\ns1,5,3,\r\n", "neither a digit nor a separator"),
    ("a-line-without-a-comma", {}, b"s0,5,3,\nnocomma\ns2,5,3,\n", "no comma"),
    ("an-empty-line", {}, b"s0,5,3,\n\ns2,5,3,\n", "no comma"),
    ("only-empty-lines", {}, b"\n\n\n", "no comma"),
    ("three-in-a-pair", {"sparse_in": True}, b"s0,5,1:2:3,\n", "':'"),
    ("a-colon-behind-the-count", {"sparse_in": True}, b"s0,5:3,1:2,\n", "':'"),
    ("phylip-from-sparse-input", {"sparse_in": True, "phylip": True}, b"s0,5,1:2,\n", "phylip"),
]


@pytest.mark.parametrize("case", DECLINED, ids=lambda c: c[0])
def test_declined_input(K, L, case):
    _, flags, text, word = case
    d = K.Distance("jaccard", 18, [10, 20, 30], **flags)
    assert d.rows(text) == (b"", K.capi.DISTANCE_DECLINED)
    assert "declined" in d.declined and word in d.declined, d.declined
    if not flags.get("phylip"):                                  # the handle stays usable
        good = b"s0,5,1:2,\n" if flags.get("sparse_in") else b"s0,5,3,\n"
        got, status = d.rows(good)
        state = {"sparse_out": True} if flags.get("sparse_in") or flags.get("sparse_out") else {}
        assert status == 0 and got == DC.Rules(L, "jaccard", 18, [10, 20, 30], **state).rows(good)
    d.close()


def test_declined_table_falls_back_to_the_host_loop(L, tmp_path):
    names = [b"a", b"b", b"c"]
    data = DC.header(18, names, [10, 20, 30]) + b"a,10,\r\nb,20,4,\r\nc,30,5,6,\r\n"
    for opts in (["jaccard"], ["-sparse", "mash"], ["-phylip-out", "ani"]):
        got, err = run_cli(tmp_path, data, opts)
        assert "the device path declined this table" in err and "neither a digit nor a separator" in err, err
        assert got == DC.distance_file(L, data, opts)
    # a later piece is declined: what the device wrote before is written again by the host loop
    data = DC.header(18, names, [10, 20, 30]) + b"a,10,1,2,3,\n" * 50 + b"b,20,-4,\n"
    got, err = run_cli(tmp_path, data, ["jaccard"], {"KMDB_DISTANCE_BYTES_PER_PIECE": "64"})
    assert "the device path declined this table" in err and got == DC.distance_file(L, data, ["jaccard"])
