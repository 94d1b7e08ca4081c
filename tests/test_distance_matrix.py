"""all2all -distance: the table of a measure straight from the matrix in HBM (kmdb_distance_take_all2all, kmdb_distance_take_cells_device,
kmdb_distance_matrix_rows; the front-end's `all2all -distance <measure>`).  The definition: byte for byte the file `all2all D T` followed by
`distance O <measure> T out` writes, T the dense table of counts.  The witness is never the code under test: the row rules restated in
tests/distance_cases.py over the dense text of the same triangle, and the reference's own golden files."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distance_cases as DC
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
ENTRIES = ("kmdb_distance_take_all2all", "kmdb_distance_take_cells_device", "kmdb_distance_matrix_rows")
FORMS = {  # name -> (flags of the device handle, state the restated loop starts in)
    "dense": ({}, {}),
    "phylip": ({"phylip": True}, {"phylip": True}),
    "sparse": ({"sparse_out": True}, {"sparse_out": True}),
}


@pytest.fixture(scope="module")
def L(K):
    lib = K.capi.lib()
    lib.kmdbh_metric.restype = ctypes.c_double
    return lib


# ---- no device -------------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_matrix_entry_points(K):
    hdr = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    assert re.search(r"^#define KMDB_HAS_DISTANCE_MATRIX 1$", hdr, re.M) and "#define KMDB_ABI_VERSION 8" in hdr and K.ABI_VERSION == 8
    lib = ctypes.CDLL(K.lib_path())
    for name in ENTRIES + ("kmdb_distance_cells_device",):
        assert hasattr(lib, name) and name in K.capi.EXPORTS and name + "(" in hdr, name


def test_null_arguments_are_refused_by_name(K):
    lib = K.capi.lib()
    assert lib.kmdb_distance_take_all2all(None, None, None, None) != 0 and b"kmdb_distance_take_all2all" in lib.kmdb_last_error()
    assert lib.kmdb_distance_take_cells_device(None, None, 0, None) != 0 and b"kmdb_distance_take_cells_device" in lib.kmdb_last_error()
    assert lib.kmdb_distance_matrix_rows(None, 0, 0, None) != 0 and b"kmdb_distance_matrix_rows" in lib.kmdb_last_error()
    assert lib.kmdb_distance_cells_device(None) is None


def cli(argv, env_extra=None):
    return subprocess.run([EXE] + [str(a) for a in argv], capture_output=True, text=True, env=dict(os.environ, **(env_extra or {})))


def test_front_end_refusals(tmp_path):
    nodb, out = tmp_path / "no-such.db", tmp_path / "out"
    r = cli(["all2all", "-distance", "nosuch", nodb, out])         # before the database is opened: the file does not exist
    assert r.returncode != 0 and "unknown measure: nosuch" in r.stderr
    r = cli(["all2all", "-gpus", "2", "-distance", "jaccard", nodb, out])
    assert r.returncode != 0 and "-distance" in r.stderr and "-gpus" in r.stderr
    for mode in ("all2all", "all2all-sp"):
        r = cli([mode, "-sample-rows", "jaccard:3", "-distance", "jaccard", nodb, out])
        assert r.returncode != 0 and "-distance" in r.stderr and "-sample-rows" in r.stderr
    r = cli(["all2all", "-phylip-out", nodb, out])                  # without -distance: the usage error it was
    assert r.returncode != 0 and "USAGE" in r.stderr
    assert not out.exists()


# ---- the library, random triangles as torch tensors ------------------------------------------------------------------------------------------
def to_device(cells):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cells, np.uint32).view(np.int32)).cuda()


def split_bounds(bounds):
    kmer = [b for b in bounds if b[0] == "num-kmers"]
    return ([b for b in bounds if b[0] != "num-kmers"], int(kmer[0][1]) if kmer and kmer[0][1] is not None else 0,
            int(kmer[0][2]) if kmer and kmer[0][2] is not None else DC.M32)


def witness(L, names, counts, rows, measure, k, form, bounds=(), first_row=0, cache=None):
    """rows: the cells of rows first_row, first_row + 1, ... of the triangle -> what `distance` writes for those rows of its dense table"""
    other, lo, hi = split_bounds(bounds)
    text = b"".join(names[first_row + i] + b",%d," % counts[first_row + i] + b"".join(b"%d," % v for v in r) + b"\n" for i, r in enumerate(rows))
    r = DC.Rules(L, measure, k, counts, bounds=other, kmer_lo=lo, kmer_hi=hi, triangle=True, cache=cache, **FORMS[form][1])
    return r.rows(text, first_row)


@pytest.fixture(scope="module")
def table70():
    """70 samples: rows cross the 64-lane wave, the 2 415 cells several workgroups.  Two samples without k-mers (a + b - c = 0: NaN, the
    host's cell), two of equal counts with a cell equal to both, 30 % zeros, one empty name and one of 80 bytes."""
    rng = np.random.default_rng(70)
    n = 70
    counts = DC.random_counts(rng, n)
    counts[5] = counts[9] = 0
    counts[20] = counts[21] = 4_000_000
    cells = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i):
            cells[i, j] = rng.integers(1, min(counts[i], counts[j]) + 1) if min(counts[i], counts[j]) and rng.random() >= 0.3 else 0
    cells[21, 20] = 4_000_000
    names = [b"s%d" % i for i in range(n)]
    names[3] = b""
    names[66] = b"a-name-of-eighty-bytes-" + b"x" * 57
    assert len(names[66]) == 80
    text = DC.dense_body(names, counts, cells, triangle=True)
    tri = np.concatenate([cells[i, :i] for i in range(n)]).astype(np.uint32)
    assert tri.size == 2415
    return {"n": n, "counts": counts, "cells": cells, "names": names, "text": text, "tri": tri, "cache": {}}


def bounds_for(L, t, measure):
    """on the measure (the median of row 40's values: about half the cells pass whichever way the measure runs), on another criterion, on the count"""
    m = DC.METRICS.index(measure)
    vals = sorted(L.kmdbh_metric(m, ctypes.c_uint32(int(c)), ctypes.c_uint32(int(t["counts"][40])), ctypes.c_uint32(int(t["counts"][j])), 21)
                  for j, c in enumerate(t["cells"][40][:40]) if c and t["counts"][j])
    other = "max" if measure != "max" else "min"
    b = [(measure, vals[len(vals) // 2], None), (other, 0.05, 0.95)]
    if measure != "num-kmers":
        b.append(("num-kmers", 1000, 4_500_000))
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("measure", DC.METRICS)
def test_every_measure_and_form_from_the_triangle(K, L, table70, measure, form):
    t = table70
    bounds = bounds_for(L, t, measure) if form == "sparse" else []
    other, lo, hi = split_bounds(bounds)
    want = DC.Rules(L, measure, 21, t["counts"], bounds=other, kmer_lo=lo, kmer_hi=hi, triangle=True, cache=t["cache"], **FORMS[form][1]).rows(t["text"])
    dev = to_device(t["tri"])
    d = K.Distance(measure, 21, t["counts"], filters=bounds, triangle=True, **FORMS[form][0])
    d.take_cells(dev.data_ptr(), 0, t["names"])
    assert d.cells_ptr() == dev.data_ptr()
    whole = d.matrix_rows(0, 70)
    assert whole == want
    pieces = [d.matrix_rows(0, 1), d.matrix_rows(1, 65), d.matrix_rows(65, 70), d.matrix_rows(70, 70)]
    assert pieces[3] == b"" and b"".join(pieces) == want
    st = d.stats()
    assert st["calls"] == 5 and st["rows"] == 140 and st["cells_read"] == 2 * 2415 and st["parse_ms"] == 0, st
    if measure in ("jaccard", "mash", "ani") and form != "sparse":
        assert st["host_cells"] >= 2, st                           # cell (9, 5): 0 / 0, once in each pass
    d.close()
    del dev


@pytest.mark.gpu
def test_one_sample_has_no_cells(K):
    for form, want in (("dense", b"only,\n"), ("sparse", b"only,\n"), ("phylip", b"only \n")):
        d = K.Distance("jaccard", 21, [5], triangle=True, **FORMS[form][0])
        d.take_cells(None, 0, [b"only"])
        assert d.matrix_rows(0, 1) == want and d.matrix_rows(0, 0) == b"" and d.matrix_rows(1, 1) == b""
        d.close()


@pytest.mark.gpu
def test_cells_on_the_rounding_boundary_are_the_hosts(K, L):
    """counts 10^6 + i and cells i + j: a + b - c = 2 000 000 for every cell, jaccard = (i + j) / 2e6, and |v| * 1e6 + 0.5 is an integer
    wherever i + j is odd — the value the sixth decimal turns on"""
    n = 40
    counts = [1_000_000 + i for i in range(n)]
    cells = np.add.outer(np.arange(n), np.arange(n))
    names = [b"b%d" % i for i in range(n)]
    tri = np.concatenate([cells[i, :i] for i in range(n)]).astype(np.uint32)
    dev = to_device(tri)
    for form in ("dense", "sparse", "phylip"):
        d = K.Distance("jaccard", 20, counts, triangle=True, **FORMS[form][0])
        d.take_cells(dev.data_ptr(), 0, names)
        got = d.matrix_rows(0, n)
        assert d.stats()["host_cells"] > 0
        assert got == witness(L, names, counts, [cells[i, :i] for i in range(n)], "jaccard", 20, form)
        d.close()


@pytest.mark.gpu
def test_late_rows_of_a_large_triangle(K, L):
    """rows 70 000 and 70 001 of 70 002 samples, handed over as their own 140 001 cells: cell 2 449 965 000 and on — 32 bits end at row 92 682,
    i (i - 1) before the halving at row 65 537"""
    n, lo = 70_002, 70_000
    rng = np.random.default_rng(7)
    counts = DC.random_counts(rng, n)
    rows = [(rng.integers(1000, 3_000_000, r) * (rng.random(r) < 0.02)).astype(np.uint32) for r in (lo, lo + 1)]
    rows[1][lo] = 12345                                              # the last cell of the triangle
    names = [b"n%d" % i for i in range(n)]
    dev = to_device(np.concatenate(rows))
    cache = {}
    for measure, form, bounds in (("jaccard", "dense", []), ("mash", "sparse", [("mash", None, 0.25)])):
        d = K.Distance(measure, 21, counts, filters=bounds, triangle=True, **FORMS[form][0])
        d.take_cells(dev.data_ptr(), lo, names)
        want = witness(L, names, counts, rows, measure, 21, form, bounds, first_row=lo, cache=cache)
        assert d.matrix_rows(lo, n) == want
        assert d.matrix_rows(lo, lo + 1) + d.matrix_rows(lo + 1, n) == want
        with pytest.raises(K.KmdbError, match="in front of the cells taken"):
            d.matrix_rows(lo - 1, n)
        d.close()


@pytest.mark.gpu
def test_refusals(K, golden_dir):
    names = [b"a", b"b", b"c"]
    dev = to_device(np.array([1, 2, 3], np.uint32))
    for flags, word in (({}, "KMDB_DISTANCE_TRIANGLE"), ({"triangle": True, "sparse_in": True}, "KMDB_DISTANCE_SPARSE_IN")):
        d = K.Distance("jaccard", 18, [10, 20, 30], **flags)
        with pytest.raises(K.KmdbError, match="kmdb_distance_take_cells_device.*" + word):
            d.take_cells(dev.data_ptr(), 0, names)
        with pytest.raises(K.KmdbError, match="kmdb_distance_matrix_rows.*" + word):
            d.matrix_rows(0, 3)
        d.close()
    d = K.Distance("jaccard", 18, [10, 20, 30], triangle=True)
    with pytest.raises(K.KmdbError, match="no matrix was taken"):
        d.matrix_rows(0, 3)
    d.take_cells(dev.data_ptr(), 0, names)
    with pytest.raises(K.KmdbError, match="row_hi 4 > 3"):
        d.matrix_rows(0, 4)
    with pytest.raises(K.KmdbError, match="row_lo > row_hi"):
        d.matrix_rows(2, 1)
    with pytest.raises(K.KmdbError, match="row_lo 4"):
        d.take_cells(dev.data_ptr(), 4, names)
    d.take_cells(None, 0, names)                                     # a null pointer is taken; rows with cells are refused, row 0 is served
    assert d.matrix_rows(0, 1) == b"a,\n"
    with pytest.raises(K.KmdbError, match="null pointer"):
        d.matrix_rows(0, 2)
    db = K.DeviceDB(K.HostDB(os.path.join(golden_dir, "synth_k21.db"), skip_hashtables=True))       # five samples, the handle has three
    with pytest.raises(K.KmdbError, match="kmdb_distance_take_all2all.*5 samples.*3"):
        d.take_all2all(db, names)
    d.close()


# ---- end to end: the reference's goldens -----------------------------------------------------------------------------------------------------
def header_of(h, phylip=False):
    return b"%d\n" % h.N if phylip else b"kmer-length: %d fraction: %s ," % (h.k, b"%g" % h.fraction) + b"".join(n.encode() + b"," for n in h.names) + b"\n"


@pytest.mark.gpu
def test_take_all2all_gives_the_virus_goldens(K, golden_dir):
    h = K.HostDB(os.path.join(golden_dir, "virus_k18.db"), skip_hashtables=True)
    db = K.DeviceDB(h)
    owner = None
    for measure in ("jaccard", "min", "max", "cosine", "mash"):
        d = K.Distance(measure, h.k, h.sample_kmers, triangle=True)
        if owner is None:
            d.take_all2all(db, h.names)
            owner = d
        else:                                                        # one all2all run serves every measure: the others borrow its cells
            d.take_cells(owner.cells_ptr(), 0, h.names)
        got = header_of(h) + d.matrix_rows(0, h.N)
        assert got == open(os.path.join(golden_dir, "virus.k18.csv." + measure), "rb").read(), measure
        st = d.stats()
        assert st["rows"] == h.N and st["cells_read"] == h.N * (h.N - 1) // 2 and st["host_cells"] < st["cells_written"]
        if d is not owner:
            d.close()
    owner.take_all2all(db, h.names)                                 # a second take frees the first triangle and gives the same table
    assert header_of(h) + owner.matrix_rows(0, h.N) == open(os.path.join(golden_dir, "virus.k18.csv.jaccard"), "rb").read()
    owner.close()


def run_a2a(tmp_path, golden_dir, db, opts, mode="all2all", env_extra=None):
    out = tmp_path / "out"
    r = cli([mode] + opts + [os.path.join(golden_dir, db), out], dict(env_extra or {}, KMDB_VERBOSE="1"))
    assert r.returncode == 0, r.stderr
    return out, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("measure", ["jaccard", "min", "max", "cosine", "mash"])
def test_cli_virus_goldens(golden_dir, tmp_path, measure):
    out, err = run_a2a(tmp_path, golden_dir, "virus_k18.db", ["-distance", measure])
    assert out.read_bytes() == open(os.path.join(golden_dir, "virus.k18.csv." + measure), "rb").read()


@pytest.mark.gpu
def test_cli_several_measures_share_one_run(golden_dir, tmp_path):
    out, err = run_a2a(tmp_path, golden_dir, "virus_k18.db", ["-distance", "jaccard", "-distance", "mash"])
    assert not out.exists()
    for measure in ("jaccard", "mash"):
        assert (tmp_path / ("out." + measure)).read_bytes() == open(os.path.join(golden_dir, "virus.k18.csv." + measure), "rb").read()
    assert err.count("Calculating matrix of common k-mers") == 1


SYNTH = [
    ("all2all", ["-distance", "mash"], "synth.a2a.mash"),
    ("all2all", ["-distance", "ani"], "synth.a2a.ani"),
    ("all2all", ["-sparse", "-distance", "ani"], "synth.a2a-sparse.ani"),
    ("all2all", ["-sparse", "-max", "1.0", "-min", "-1.0", "-distance", "mash"], "synth.a2a-sparse.mash"),
    ("all2all", ["-sparse", "-min", "0.03", "-max", "mash:1.0", "-min", "num-kmers:36", "-distance", "mash"], "synth.a2a.mash-sparse-min2max"),
    ("all2all-sp", ["-distance", "ani"], "synth.a2a-sparse.ani"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SYNTH, ids=lambda c: c[0] + ":" + "_".join(c[1]))
def test_cli_synth_goldens(golden_dir, tmp_path, case):
    mode, opts, want = case
    out, err = run_a2a(tmp_path, golden_dir, "synth_k21.db", opts, mode)
    assert out.read_bytes() == open(os.path.join(golden_dir, want), "rb").read()


@pytest.mark.gpu
def test_cli_phylip_and_the_fraction_in_the_header(L, golden_dir, tmp_path):
    src = os.path.join(golden_dir, "virus.k18.frac.csv")
    for opts in ([], ["-phylip-out"], ["-sparse", "-min", "0.5"]):
        want = tmp_path / "want"
        r = cli(["distance", "-host"] + opts + ["jaccard", src, want])
        assert r.returncode == 0, r.stderr
        out, err = run_a2a(tmp_path, golden_dir, "virus_k18_f01.db", opts + ["-distance", "jaccard"])
        assert out.read_bytes() == want.read_bytes(), opts
        assert want.read_bytes() == DC.distance_file(L, open(src, "rb").read(), opts + ["jaccard"])
    assert b"fraction: 0.1 ," in out.read_bytes().split(b"\n")[0]


@pytest.mark.gpu
def test_cli_pieces_of_a_thousand_cells(golden_dir, tmp_path):
    out, err = run_a2a(tmp_path, golden_dir, "virus_k18.db", ["-distance", "jaccard"], env_extra={"KMDB_DISTANCE_CELLS_PER_PIECE": "1000"})
    assert out.read_bytes() == open(os.path.join(golden_dir, "virus.k18.csv.jaccard"), "rb").read()
    m = re.search(r"distance from the matrix: calls (\d+), rows (\d+), cells read (\d+)", err)
    n = int(m.group(2))
    assert int(m.group(3)) == n * (n - 1) // 2 and int(m.group(1)) >= int(m.group(3)) // 1000 and int(m.group(1)) > 1, err
