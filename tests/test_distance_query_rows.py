"""new2all -distance: the table of a measure straight from the rows of a batch of queries in HBM (kmdb_distance_take_new2all_batch,
kmdb_distance_take_new2all_batch_seq_alphabet, kmdb_distance_take_rows_device, kmdb_distance_query_rows; the front-end's
`new2all -distance <measure>`).  The definition: byte for byte the file `new2all D Q T` followed by `distance -host <measure> T out` writes, T
the dense table of counts.  The witness is never the code under test: the row rules restated in tests/distance_cases.py over the dense text
of the same rectangle, the host loop run on the reference's recorded tables, and the reference's own golden files."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distance_cases as DC
import distance_query_cases as QC
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
ENTRIES = ("kmdb_distance_take_new2all_batch", "kmdb_distance_take_new2all_batch_seq_alphabet", "kmdb_distance_take_rows_device", "kmdb_distance_query_rows")
FORMS = QC.FORMS


@pytest.fixture(scope="module")
def L(K):
    lib = K.capi.lib()
    lib.kmdbh_metric.restype = ctypes.c_double
    return lib


@pytest.fixture(scope="module")
def table9x70():
    """630 cells: rows end inside 64-lane waves and inside 256-thread workgroups.  It holds no query or sample without k-mers and no cell on a
    rounding boundary (test_the_table_has_no_cell_within_the_host_margins): those have tables of their own."""
    return QC.table(9, 70, 970)


# ---- no device -------------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_query_row_entry_points(K):
    hdr = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    assert re.search(r"^#define KMDB_HAS_DISTANCE_QUERY_ROWS 1$", hdr, re.M) and "#define KMDB_ABI_VERSION 8" in hdr and K.ABI_VERSION == 8
    lib = K.capi.lib()                                              # (the loader's own handle: it brings torch's HIP runtime in first)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in K.capi.EXPORTS and name + "(" in hdr, name


def test_null_arguments_are_refused_by_name(K):
    lib = K.capi.lib()
    assert lib.kmdb_distance_take_new2all_batch(None, None, None, None, 0, None, None) != 0 and b"kmdb_distance_take_new2all_batch:" in lib.kmdb_last_error()
    assert lib.kmdb_distance_take_new2all_batch_seq_alphabet(None, None, None, None, 0, 1.0, 0.0, 0, None, None, None) != 0
    assert b"kmdb_distance_take_new2all_batch_seq_alphabet:" in lib.kmdb_last_error()
    assert lib.kmdb_distance_take_rows_device(None, None, 0, None, None) != 0 and b"kmdb_distance_take_rows_device:" in lib.kmdb_last_error()
    assert lib.kmdb_distance_query_rows(None, 0, 0, None) != 0 and b"kmdb_distance_query_rows:" in lib.kmdb_last_error()


def cli(argv, env_extra=None, cwd=None):
    return subprocess.run([EXE] + [str(a) for a in argv], capture_output=True, text=True, env=dict(os.environ, **(env_extra or {})), cwd=cwd)


def test_front_end_refusals(tmp_path):
    nodb, lst, out = tmp_path / "no-such.db", tmp_path / "no-such.list", tmp_path / "out"
    r = cli(["new2all", "-distance", "nosuch", nodb, lst, out])     # before the database is opened: the file does not exist
    assert r.returncode != 0 and "unknown measure: nosuch" in r.stderr
    r = cli(["new2all", "-gpus", "2", "-distance", "jaccard", nodb, lst, out])
    assert r.returncode != 0 and "-distance" in r.stderr and "-gpus" in r.stderr and "no-such" not in r.stderr
    r = cli(["one2all", "-distance", "jaccard", nodb, lst, out])
    assert r.returncode != 0 and "one2all" in r.stderr and "-distance" in r.stderr and "USAGE" not in r.stderr and "no-such" not in r.stderr
    r = cli(["new2all", "-phylip-out", nodb, lst, out])             # without -distance: the usage error it was
    assert r.returncode != 0 and "USAGE" in r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".jaccard")
    assert "-distance <measure> [-distance <measure>]* <database> <sample_list> <output>" in cli([]).stderr


def test_the_table_has_no_cell_within_the_host_margins(L, table9x70):
    """what lets test_the_host_cannot_carry_the_table ask for (nearly) no host cells: decided on the CPU, with kmdbh_metric"""
    for measure in DC.METRICS:
        assert QC.host_margin_cells(L, table9x70, measure) == [], measure


# ---- the library, rectangles as torch tensors --------------------------------------------------------------------------------------------------
def to_device(cells):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cells, np.uint32).view(np.int32)).cuda()


def handle(K, t, measure, form, bounds=()):
    return K.Distance(measure, QC.K_LEN, t["counts"], filters=bounds, **FORMS[form][0])


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("measure", DC.METRICS)
def test_every_measure_and_form_from_the_rows(K, L, table9x70, measure, form):
    t = table9x70
    bounds = QC.bounds_for(L, t, measure) if form == "sparse" else []
    want = QC.witness(L, t, measure, form, bounds)
    dev = to_device(t["flat"])
    d = handle(K, t, measure, form, bounds)
    d.take_rows(dev.data_ptr(), 9, t["query_counts"], t["names"])
    assert d.cells_ptr() == dev.data_ptr()
    whole = d.query_rows(0, 9)
    assert whole == want
    pieces = [d.query_rows(0, 1), d.query_rows(1, 4), d.query_rows(4, 9), d.query_rows(9, 9)]
    assert pieces[3] == b"" and b"".join(pieces) == want
    st = d.stats()
    assert st["calls"] == 5 and st["rows"] == 18 and st["cells_read"] == 2 * 630 and st["bytes_in"] == 8 * 630 and st["parse_ms"] == 0, st
    d.close()
    del dev


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("nq,n", [(5, 64), (3, 256), (1, 1)])
def test_rows_that_end_on_wave_and_workgroup_borders(K, L, nq, n, form):
    t = QC.table(nq, n, 1000 * nq + n)
    dev = to_device(t["flat"])
    for measure in ("jaccard", "cosine", "mash-query"):
        bounds = QC.bounds_for(L, t, measure) if form == "sparse" and n > 1 else []
        d = handle(K, t, measure, form, bounds)
        d.take_rows(dev.data_ptr(), nq, t["query_counts"], t["names"])
        assert d.query_rows(0, nq) == QC.witness(L, t, measure, form, bounds), measure
        if nq > 1:
            assert d.query_rows(1, nq) == QC.witness(L, t, measure, form, bounds, rows=(1, nq)), measure
        d.close()


@pytest.mark.gpu
def test_counts_of_zero_are_the_hosts(K, L):
    t = QC.zero_counts()
    dev = to_device(t["flat"])
    for measure in ("jaccard", "min", "mash-query", "ani-shorter"):
        for form in ("dense", "sparse", "phylip"):
            d = handle(K, t, measure, form)
            d.take_rows(dev.data_ptr(), t["nq"], t["query_counts"], t["names"])
            assert d.query_rows(0, t["nq"]) == QC.witness(L, t, measure, form), (measure, form)
            if form != "sparse":                                     # (the sparse form leaves the cells of count 0 out: most of these)
                assert d.stats()["host_cells"] > 0, (measure, form)
            d.close()


@pytest.mark.gpu
def test_a_cell_on_the_rounding_boundary_is_the_hosts(K, L):
    t = QC.rounding_boundary()
    dev = to_device(t["flat"])
    for form in ("dense", "sparse", "phylip"):
        d = handle(K, t, "max", form)
        d.take_rows(dev.data_ptr(), t["nq"], t["query_counts"], t["names"])
        got = d.query_rows(0, t["nq"])
        assert got == QC.witness(L, t, "max", form), form
        assert d.stats()["host_cells"] >= 1
        d.close()
    assert b"r0,0.000001,0.000001," in QC.witness(L, t, "max", "dense")


@pytest.mark.gpu
@pytest.mark.parametrize("measure", DC.METRICS)
def test_the_host_cannot_carry_the_table(K, L, table9x70, measure):
    t = table9x70
    dev = to_device(t["flat"])
    d = handle(K, t, measure, "dense")
    d.take_rows(dev.data_ptr(), 9, t["query_counts"], t["names"])
    assert d.query_rows(0, 9) == QC.witness(L, t, measure, "dense")
    st = d.stats()
    assert st["cells_written"] == 630 and st["host_cells"] * 100 <= st["cells_written"], st
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("measure", ["jaccard", "mash"])
def test_the_text_path_gives_the_same_bytes(K, L, table9x70, measure, form):
    t = table9x70
    bounds = QC.bounds_for(L, t, measure) if form == "sparse" else []
    dev = to_device(t["flat"])
    d = handle(K, t, measure, form, bounds)
    d.take_rows(dev.data_ptr(), 9, t["query_counts"], t["names"])
    text = handle(K, t, measure, form, bounds)
    got, rc = text.rows(t["text"])
    assert rc == 0 and got == d.query_rows(0, 9) == QC.witness(L, t, measure, form, bounds)
    d.close()
    text.close()


@pytest.mark.gpu
def test_a_second_handle_borrows_the_rows(K, L, table9x70):
    t = table9x70
    dev = to_device(t["flat"])
    first = handle(K, t, "jaccard", "dense")
    first.take_rows(dev.data_ptr(), 9, t["query_counts"], t["names"])
    bounds = QC.bounds_for(L, t, "ani")
    second = handle(K, t, "ani", "sparse", bounds)
    second.take_rows(first.cells_ptr(), 9, t["query_counts"], t["names"])
    assert second.query_rows(0, 9) == QC.witness(L, t, "ani", "sparse", bounds)
    assert first.query_rows(0, 9) == QC.witness(L, t, "jaccard", "dense")
    first.close()
    second.close()


@pytest.mark.gpu
def test_refusals(K, golden_dir):
    names = [b"a", b"b"]
    dev = to_device(np.arange(1, 7, dtype=np.uint32))
    for flags, word in (({"triangle": True}, "KMDB_DISTANCE_TRIANGLE"), ({"sparse_in": True}, "KMDB_DISTANCE_SPARSE_IN")):
        d = K.Distance("jaccard", 18, [10, 20, 30], **flags)
        with pytest.raises(K.KmdbError, match="kmdb_distance_take_rows_device.*" + word):
            d.take_rows(dev.data_ptr(), 2, [7, 8], names)
        with pytest.raises(K.KmdbError, match="kmdb_distance_query_rows.*" + word):
            d.query_rows(0, 2)
        d.close()
    d = K.Distance("num-kmers", 18, [10, 20, 30])
    with pytest.raises(K.KmdbError, match="kmdb_distance_query_rows: no rows were taken"):
        d.query_rows(0, 2)
    assert d.cells_ptr() is None
    d.take_rows(dev.data_ptr(), 2, [7, 8], names)
    with pytest.raises(K.KmdbError, match="row_hi 3 > 2"):
        d.query_rows(0, 3)
    with pytest.raises(K.KmdbError, match="row_lo > row_hi"):
        d.query_rows(2, 1)
    assert d.query_rows(0, 2) == b"a,1.000000,2.000000,3.000000,\nb,4.000000,5.000000,6.000000,\n"      # the handle stays usable
    d.take_rows(None, 2, [7, 8], names)                              # a null pointer is taken; rows with cells are refused
    assert d.query_rows(1, 1) == b""
    with pytest.raises(K.KmdbError, match="kmdb_distance_query_rows.*6 cells and a null pointer"):
        d.query_rows(0, 2)
    path = os.path.join(golden_dir, "synth_k21.db")                  # five samples, the handle has three
    h = K.HostDB(path)
    db = K.DeviceDB(h, with_hashtables=True)
    q = [np.array([1, 2, 3], np.uint64), np.array([5], np.uint64)]
    with pytest.raises(K.KmdbError, match="kmdb_distance_take_new2all_batch: .*5 samples.*3"):
        d.take_new2all(db, q, names)
    with pytest.raises(K.KmdbError, match="kmdb_distance_take_new2all_batch_seq_alphabet: .*5 samples.*3"):
        d.take_new2all_seqs(db, ["ACGT", "ACGT"], names)
    d.take_rows(dev.data_ptr(), 2, [7, 8], names)
    assert d.query_rows(1, 2) == b"b,4.000000,5.000000,6.000000,\n"
    d.close()
    d = K.Distance("jaccard", h.k, h.sample_kmers)
    shard = K.DeviceDB(h, query_shard=(0, 2))
    with pytest.raises(K.KmdbError, match="kmdb_distance_take_new2all_batch: a query shard"):
        d.take_new2all(shard, q, names)
    shard.close()
    bare = K.DeviceDB(K.HostDB(path, skip_hashtables=True))
    with pytest.raises(K.KmdbError, match="kmdb_distance_take_new2all_batch: .*without hashtables"):
        d.take_new2all(bare, q, names)
    bare.close()
    d.take_new2all(db, q, names)                                     # and the handle serves a database that fits it
    assert d.query_rows(0, 2).count(b"\n") == 2
    d.close()
    db.close()


# ---- the library on the reference's recorded table ---------------------------------------------------------------------------------------------
def virus_texts(golden_dir, list_name):
    """sequence text of the genomes of a sample list: the records of one file joined by a newline"""
    texts = []
    with open(os.path.join(golden_dir, list_name)) as f:
        entries = [ln.strip() for ln in f if ln.strip()]
    for e in entries:
        raw = open(os.path.join(golden_dir, e + ".fasta")).read()
        recs = [r.split("\n", 1)[1] if "\n" in r else "" for r in raw.split(">") if r]
        texts.append("\n".join(r.replace("\n", "").replace("\r", "") for r in recs))
    return texts


@pytest.mark.gpu
def test_take_new2all_gives_the_rows_of_the_virus_golden(K, L, golden_dir):
    k, fraction, rest, names, counts, body = DC.parse_table(open(os.path.join(golden_dir, "virus.k18.n2a.csv"), "rb").read())
    lines = body.split(b"\n")[:-1]
    qnames = [ln.split(b",")[0] for ln in lines]
    h = K.HostDB(os.path.join(golden_dir, "virus_k18_part1.db"))
    assert (h.k, h.N, len(lines)) == (k, len(counts), 65) and [int(c) for c in h.sample_kmers] == counts
    db = K.DeviceDB(h, with_hashtables=True)
    texts = virus_texts(golden_dir, "virus.seqs.part2.list")
    lists = [K.sort_unique(np.concatenate([K.extract_kmers(rec, k, 1.0) for rec in t.split("\n")])) for t in texts]
    cache = {}
    for measure, form, bounds in (("jaccard", "dense", []), ("mash", "sparse", [("mash", None, 0.05)])):
        rules = lambda: DC.Rules(L, measure, k, counts, bounds=bounds, triangle=False, cache=cache, **FORMS[form][1])      # noqa: E731
        want = rules().rows(body)
        d = K.Distance(measure, k, h.sample_kmers, filters=bounds, **FORMS[form][0])
        d.take_new2all(db, lists, qnames)
        assert d.query_rows(0, 65) == want, (measure, form, "k-mer lists")
        assert d.query_rows(0, 30) + d.query_rows(30, 65) == want
        uniq = d.take_new2all_seqs(db, texts, qnames)
        assert [int(u) for u in uniq] == [x.size for x in lists]
        assert d.query_rows(0, 65) == want, (measure, form, "text")
        # a smaller batch on the same handle: the rectangle is kept, zeroed again, and rows 60 .. 64 become rows 0 .. 4
        d.take_new2all(db, lists[60:], qnames[60:])
        assert d.query_rows(0, 5) == rules().rows(b"".join(ln + b"\n" for ln in lines[60:]), 60)
        with pytest.raises(K.KmdbError, match="row_hi 6 > 5"):
            d.query_rows(0, 6)
        st = d.stats()
        assert st["cells_read"] == (65 + 65 + 65 + 5) * h.N and st["host_cells"] < st["cells_written"], st
        d.close()
    db.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def run_n2a(tmp_path, golden_dir, db, lst, opts, env_extra=None, name="out"):
    out = tmp_path / name
    r = cli(["new2all"] + opts + [os.path.join(golden_dir, db), lst, out], dict(env_extra or {}, KMDB_VERBOSE="1"), cwd=golden_dir)   # the list entries are ./test/virus/data/<name>
    assert r.returncode == 0, r.stderr
    return out, r.stderr


def host_distance(tmp_path, golden_dir, table, opts, measure):
    want = tmp_path / "want"
    r = cli(["distance", "-host"] + opts + [measure, os.path.join(golden_dir, table), want])
    assert r.returncode == 0, r.stderr
    return want.read_bytes()


SYNTH = [
    (["-distance", "mash"], "synth.n2a.mash"),
    (["-distance", "ani"], "synth.n2a.ani"),
    (["-sparse", "-distance", "ani"], "synth.n2a-sparse.ani"),
    (["-sparse", "-max", "1.0", "-min", "-1.0", "-distance", "mash"], "synth.n2a-sparse.mash"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SYNTH, ids=lambda c: "_".join(c[0]))
def test_cli_synth_goldens(golden_dir, tmp_path, case):
    opts, want = case
    lst = tmp_path / "synth.list"
    lst.write_text(os.path.join(golden_dir, "synth.synth") + "\n")
    out, err = run_n2a(tmp_path, golden_dir, "synth_k21.db", lst, ["-multisample-fasta"] + opts)
    assert out.read_bytes() == open(os.path.join(golden_dir, want), "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("opts,measure", [([], "jaccard"), ([], "cosine"), (["-phylip-out"], "ani")], ids=["jaccard", "cosine", "phylip-ani"])
def test_cli_virus_part2_against_part1(L, golden_dir, tmp_path, opts, measure):
    want = host_distance(tmp_path, golden_dir, "virus.k18.n2a.csv", opts, measure)
    assert want == DC.distance_file(L, open(os.path.join(golden_dir, "virus.k18.n2a.csv"), "rb").read(), opts + [measure])
    lst = os.path.join(golden_dir, "virus.seqs.part2.list")
    out, err = run_n2a(tmp_path, golden_dir, "virus_k18_part1.db", lst, opts + ["-distance", measure])
    assert out.read_bytes() == want
    m = re.search(r"distance from the query rows: calls (\d+), rows (\d+), cells read (\d+)", err)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (2, 65, 6500), err       # 65 queries: a batch of 64 and one of 1
    out, err = run_n2a(tmp_path, golden_dir, "virus_k18_part1.db", lst, opts + ["-distance", measure], {"KMDB_DISTANCE_CELLS_PER_PIECE": "150"}, "out.150")
    assert out.read_bytes() == want
    m = re.search(r"distance from the query rows: calls (\d+), rows (\d+), cells read (\d+)", err)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (65, 65, 6500), err      # a row of 100 cells a piece
    out, err = run_n2a(tmp_path, golden_dir, "virus_k18_part1.db", lst, opts + ["-host-extract", "-distance", measure], name="out.host")
    assert out.read_bytes() == want


@pytest.mark.gpu
def test_cli_several_measures_share_one_run(golden_dir, tmp_path):
    lst = os.path.join(golden_dir, "virus.seqs.part2.list")
    out, err = run_n2a(tmp_path, golden_dir, "virus_k18_part1.db", lst, ["-sparse", "-min", "0.9", "-distance", "jaccard", "-distance", "max"])
    assert not out.exists()
    for measure in ("jaccard", "max"):                               # the bare bound belongs to the measure of each table
        want = host_distance(tmp_path, golden_dir, "virus.k18.n2a.csv", ["-sparse", "-min", "0.9"], measure)
        assert (tmp_path / ("out." + measure)).read_bytes() == want, measure
    assert err.count("Loading k-mer database") == 1


@pytest.mark.gpu
def test_cli_a_database_against_itself_is_no_triangle(golden_dir, tmp_path):
    """query 0 is named like sample 0 and its first cell is its own k-mer count, not 0: whole rows"""
    table = open(os.path.join(golden_dir, "virus.k18.n2a.itself.csv"), "rb").read()
    k, fraction, rest, names, counts, body = DC.parse_table(table)
    row0 = body.split(b"\n")[0].split(b",")
    assert row0[0] == names[0] and int(row0[2]) > 0
    want = host_distance(tmp_path, golden_dir, "virus.k18.n2a.itself.csv", [], "jaccard")
    out, err = run_n2a(tmp_path, golden_dir, "virus_k18.db", os.path.join(golden_dir, "virus.seqs.list"), ["-distance", "jaccard"])
    assert out.read_bytes() == want
    assert want.split(b"\n")[1].count(b",") == len(counts) + 1


@pytest.mark.gpu
def test_cli_the_triangle_rule_is_a_refusal(L, tmp_path):
    """the first sample of the database carries the first query's name and shares no k-mer with it: `distance` would take the dense table for
    a triangle and cut its rows; the sparse form is not affected"""
    rng = np.random.default_rng(16)
    seq = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))      # noqa: E731
    s_first, s_second, q_first = seq(300), seq(300), seq(300)
    (tmp_path / "db.fa").write_text(">first\n%s\n>second\n%s\n" % (s_first, s_second))
    (tmp_path / "q.fa").write_text(">first\n%s\n>other\n%s\n" % (q_first, s_second[:200] + q_first[:100]))
    (tmp_path / "db.list").write_text(str(tmp_path / "db.fa") + "\n")
    (tmp_path / "q.list").write_text(str(tmp_path / "q.fa") + "\n")
    db = tmp_path / "t.db"
    r = cli(["build", "-multisample-fasta", "-k", "18", tmp_path / "db.list", db])
    assert r.returncode == 0, r.stderr
    table = tmp_path / "table"
    r = cli(["new2all", "-multisample-fasta", db, tmp_path / "q.list", table])
    assert r.returncode == 0, r.stderr
    rows = table.read_bytes().split(b"\n")[2:4]
    assert re.match(rb"first,\d+,0,0,$", rows[0]) and rows[1].startswith(b"other,"), rows
    out = tmp_path / "out"
    for opts in ([], ["-phylip-out"]):
        r = cli(["new2all", "-multisample-fasta"] + opts + ["-distance", "jaccard", db, tmp_path / "q.list", out])
        assert r.returncode != 0 and "first" in r.stderr and "triangle" in r.stderr and "new2all and distance" in r.stderr, r.stderr
        assert "the first query, first, is named like the first sample of the database, first," in r.stderr and not out.exists()
    r = cli(["new2all", "-multisample-fasta", "-sparse", "-distance", "jaccard", db, tmp_path / "q.list", out])
    assert r.returncode == 0, r.stderr
    want = tmp_path / "want"
    r = cli(["distance", "-host", "-sparse", "jaccard", table, want])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == want.read_bytes() == DC.distance_file(L, table.read_bytes(), ["-sparse", "jaccard"])
    assert b"other,2:" in out.read_bytes()
