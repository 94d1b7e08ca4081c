"""kmdb_build_finish_device (KMDB_HAS_BUILD_HANDOFF): a finished builder handed to the engine in HBM, and the front-end's
`all2all | all2all-sp -from-samples`.  What defines the result is the detour it replaces: finish() + DeviceDB(h) of an identically fed builder,
and `build` followed by the table mode on the built file."""
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import build_cases as BC
import extend_cases as EC
import minhash_cases as MC
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
HEADER = os.path.join(ROOT, "include", "kmdb_amd.h")
BUILD_DIR = os.path.join(ROOT, "kmer-db_amd", "build")
NEW_SYMBOLS = ("kmdb_build_finish_device", "kmdb_build_handoff_stats_get", "kmdbh_db_header_only")
STAT_KEYS = ("n_patterns", "algorithmic_bytes", "tree_updates", "sum_pairs", "n_segments", "path", "width")


def _cli(*args, cwd=None, ok=True):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, cwd=cwd)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def _slug(text):
    return re.sub(r"\W+", "-", text)[:40]


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_declared(K):
    import ctypes
    src = EC.read(HEADER).decode()
    assert re.search(r"^#define KMDB_HAS_BUILD_HANDOFF 1$", src, re.M)
    assert re.search(r"^#define KMDB_ABI_VERSION 8$", src, re.M)
    assert K.ABI_VERSION == 8 and K.lib().kmdb_abi_version() == 8
    L = ctypes.CDLL(K.lib_path())
    for name in NEW_SYMBOLS:
        assert name in K.capi.EXPORTS and hasattr(L, name), name
        assert re.search(r"^int\s+%s\(" % name, src, re.M), name
    # the struct of the binding is the struct of the header
    m = re.search(r"typedef struct kmdb_build_handoff_stats \{(.*?)\} kmdb_build_handoff_stats;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decl = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|uint32_t|double)\s+([^;]+);", body) for n in names.split(",")]
    ctype = {"c_ulong": "uint64_t", "c_uint": "uint32_t", "c_double": "double"}
    assert decl == [(ctype[t.__name__], f) for f, t in K.capi._BuildHandoffStats._fields_]
    assert hasattr(K.Builder, "finish_device") and hasattr(K.Builder, "handoff_stats")


def test_a_header_only_image_is_refused_with_a_message(K, golden_dir, tmp_path):
    """names and counts stay readable; store and every upload say what the image is instead of writing or reading nothing"""
    full = K.HostDB(os.path.join(golden_dir, "virus_k18_part1.db"))
    h = full.header_only()
    assert (h.N, h.k, h.fraction, h.start_fraction, h.alphabet, h.names) == (full.N, full.k, full.fraction, full.start_fraction, full.alphabet, full.names)
    assert np.array_equal(h.sample_kmers, full.sample_kmers)
    v = h.view.contents
    assert int(v.n_patterns) == 0 and int(v.n_samples) == full.N and int(v.n_buckets) == 0
    out = str(tmp_path / "none.db")
    with pytest.raises(K.KmdbError, match="kmdbh_db_store: a header-only image"):
        h.store(out)
    assert not os.path.exists(out)
    for kw in ({}, {"with_hashtables": True}, {"prefix_shard": (0, 2)}, {"tree_range": (0, 2)}, {"query_shard": (0, 2)}):
        with pytest.raises(K.KmdbError, match="holds no pattern"):
            K.DeviceDB(h, **kw)


def test_cli_refusals_and_usage(tmp_path):
    """refused by name before any file is read or any device touched: exit status, the switch in the message, nothing written, and the list
    (which does not exist) never mentioned"""
    lst, out, db = str(tmp_path / "no_such.list"), str(tmp_path / "out.csv"), str(tmp_path / "kept.db")
    for mode in ("all2all", "all2all-sp"):
        for args, words in (((mode, "-from-samples", "-gpus", "2", lst, out), ("-from-samples", "-gpus")),
                            ((mode, "-from-samples", "-from-kmers", lst, out), ("KMC k-mer input (-from-kmers) is not supported",)),
                            ((mode, "-from-samples", "-extend", lst, out), ("-from-samples", "-extend")),
                            ((mode, "-from-samples", "-keep-db", db, "-extend", lst, out), ("-from-samples", "-extend")),
                            ((mode, "-keep-db", db, lst, out), ("-keep-db", "-from-samples")),
                            ((mode, "-from-samples", "-alphabet", "klingon", lst, out), ("Unknown alphabet",)),
                            ((mode, "-from-samples", "-k", "32", lst, out), ("K-mer length for the given alphabet cannot exceed 31",))):
            r = _cli(*args, ok=False)
            assert r.returncode not in (0, -11, -6), (args, r.stderr)
            err = [ln for ln in r.stderr.splitlines() if ln.startswith("ERROR: ")]
            assert len(err) == 1 and all(w in err[0] for w in words), (args, r.stderr)
            assert "no_such.list" not in r.stderr and "Unable to open" not in r.stderr, (args, r.stderr)
            assert not os.path.exists(out) and not os.path.exists(db), args
    for mode in ("new2all", "one2all", "build", "all2all-parts"):
        r = _cli(mode, "-keep-db", db, lst, out, ok=False)
        assert r.returncode != 0 and "-keep-db" in r.stderr and not os.path.exists(db)
    r = _cli("all2all", "-from-samples", lst, ok=False)              # a missing argument
    assert r.returncode != 0 and "USAGE" in r.stderr
    r = _cli("all2all", "-from-samples", "-k", "18", lst, out, ok=False)
    assert r.returncode != 0 and "Unable to open input file " + lst in r.stderr
    usage = _cli().stderr
    for line in ("    kmer-db-amd all2all | all2all-sp -from-samples [build's input switches] [-keep-db <database>] [the mode's own switches] <sample_list | fasta> <output>",
                 "-k -f -f-start -alphabet -preserve-strand -multisample-fasta -from-minhash -host-extract -extend-from <old.db>;",
                 "Refused with -gpus <N>, -from-kmers and -extend; -keep-db needs -from-samples.",
                 "Not offered: new2all / one2all -from-samples, all2all-parts, any -gpus."):
        assert line in usage, line
    # the lines that were there stay as they were
    for line in ("    kmer-db-amd all2all [-sparse [-min [<criterion>:]<v>] [-max [<criterion>:]<v>]] <database> <common_table>",
                 "    kmer-db-amd all2all-sp [-min ...] [-max ...] <database> <common_table>",
                 "    kmer-db-amd build [-k <kmer-length>] [-f <fraction>] [-f-start <v>] [-alphabet <name>] [-preserve-strand] [-multisample-fasta] [-host-extract] <sample_list | fasta> <database>",
                 "    kmer-db-amd build -from-minhash <sample_list> <database>",
                 "    kmer-db-amd build -extend-from <old.db> [-from-minhash] [-multisample-fasta] [-host-extract] <sample_list | fasta> <database>",
                 "Common options: -t <threads>, -gpu <device>",
                 "                   fraction and alphabet; <database> may be <old.db>); -extend and -from-kmers are refused",
                 "    kmer-db-amd all2all | all2all-sp [-sparse] [-phylip-out] [-min [<criterion>:]<v>]* [-max [<criterion>:]<v>]* -distance <measure> [-distance <measure>]* <database> <output>",
                 "                                  Refused with -gpus <N> and with -sample-rows.",
                 "                                  all2all-parts.  Refused with -sample-rows and with -phylip-out."):
        assert line in usage, line


def test_layout_kernels_use_no_scratch():
    """the compiler's resource remarks of layout.hip: the fields kernel of the hand-off with a scratch size of 0 and no spilled register"""
    res = os.path.join(BUILD_DIR, "layout.resources.txt")
    if not os.path.isdir(BUILD_DIR):
        pytest.skip("the build directory %s is absent" % BUILD_DIR)
    assert os.path.exists(res), "%s is missing: the build writes it for every .hip source" % res
    found, cur = {}, None
    with open(res, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.match(r"_ZN12_GLOBAL__N_1\d+(lay_\w+_kernel)E", m.group(1))
                cur = found.setdefault(k.group(1), {}) if k else None
                continue
            m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
    src = EC.read(os.path.join(ROOT, "kmer-db_amd", "csrc", "layout.hip")).decode()
    assert set(found) == set(re.findall(r"\bvoid (lay_\w+_kernel)\(", src))
    for key in ("lay_fields_kernel", "lay_copy_bits_kernel"):
        r = found[key]
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
    import importlib
    return importlib.import_module("kmerdb_amd.synth")


@pytest.fixture(scope="module")
def shape_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("handoff_shapes"))


def _feed_lists(names, lists):
    return lambda b: b.add_kmers(names, lists)


def _both(K, make, feed, tables, dev, host_image=False):
    """two builders fed identically: (handle of finish() + DeviceDB, handle of finish_device, the host image of each, hand-off stats)"""
    b1, b2 = make(), make()
    try:
        feed(b1)
        feed(b2)
        h1 = b1.finish()
        d1 = K.DeviceDB(h1, device=dev, with_hashtables=tables)
        d2, h2 = b2.finish_device(with_hashtables=tables, host_image=host_image)
        hs = b2.handoff_stats()
        return d1, d2, h1, h2, hs
    finally:
        b1.close()
        b2.close()


def _same_handles(d1, d2, h1, h2, hs, tables, queries, triangle=True, oracle=None):
    assert (d2.N, d2.P) == (d1.N, d1.P)
    assert h2.names == h1.names and np.array_equal(h2.sample_kmers, h1.sample_kmers)
    assert (h2.k, h2.fraction, h2.start_fraction, h2.alphabet) == (h1.k, h1.fraction, h1.start_fraction, h1.alphabet)
    if triangle:
        m1, m2 = d1.all2all_dense(), d2.all2all_dense()
        assert np.array_equal(m1, m2)
        if oracle is not None:
            assert np.array_equal(m2, oracle.all2all_dense())
    if tables:
        r1, r2 = d1.new2all(queries), d2.new2all(queries)
        assert np.array_equal(r1, r2)
        if oracle is not None:
            assert np.array_equal(r2, np.stack([oracle.one2all(q) for q in queries]))
    s1, s2 = d1.stats(), d2.stats()
    for key in STAT_KEYS:
        assert s1[key] == s2[key], (key, s1[key], s2[key])
    assert s2["h2d_bytes"] == 0 and s1["h2d_bytes"] > 0
    assert s2["device_bytes"] == s1["device_bytes"]
    assert hs["patterns"] == d1.P and hs["samples"] == d1.N and hs["with_hashtables"] == int(tables)
    assert hs["peak_device_bytes"] >= hs["handle_device_bytes"] > 0 and hs["total_ms"] > 0
    assert (hs["tables_ms"] > 0) == bool(tables or hs["host_image"])


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [False, True], ids=["all2all", "tables"])
@pytest.mark.parametrize("case", BC.TREES, ids=[_slug(t[0]) for t in BC.TREES])
def test_rules_of_the_tree(K, dev, case, tables):
    """2 - 7 patterns: empty samples first / middle / last, a parent left with no k-mers, ids ranked by old id"""
    what, lists, expected = case
    names = ["s%d" % i for i in range(len(lists))]
    arrs = [np.array(x, dtype=np.uint64) for x in lists]
    d1, d2, h1, h2, hs = _both(K, lambda: K.Builder(18), _feed_lists(names, arrs), tables, dev)
    assert d2.P == len(expected) and int(h2.view.contents.n_patterns) == 0
    _same_handles(d1, d2, h1, h2, hs, tables, [a for a in arrs if a.size][:3] + [np.array(sorted(BC.KM), np.uint64)])
    d1.close()
    d2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [False, True], ids=["all2all", "tables"])
@pytest.mark.parametrize("case", BC.gamma_cases(), ids=[_slug(c[0]) for c in BC.gamma_cases()])
def test_gamma_streams_at_their_edges(K, dev, case, tables):
    """streams that end at bit 64, 128 and 129, a code across a word, three streams each padded on its own, 200 one-bit codes, a 33-bit
    code: the source positions 64 * data_offset and the tail mask of the re-pack.  70 000 samples: no triangle (9.8 GB), stats and rows"""
    what, n, samples, expected = case
    names = ["s%d" % i for i in range(n)]
    empty = np.zeros(0, np.uint64)
    lists = [np.array(samples[s], dtype=np.uint64) if s in samples else empty for s in range(n)]
    d1, d2, h1, h2, hs = _both(K, lambda: K.Builder(18), _feed_lists(names, lists), tables, dev)
    qs = [np.array(sorted(BC.KM), np.uint64), np.array([BC.a, BC.b, BC.c], np.uint64), np.array([BC.d], np.uint64)]
    _same_handles(d1, d2, h1, h2, hs, tables, qs, triangle=n < 5000)
    if tables and n >= 5000:
        row = d2.new2all(qs[1:2])[0]
        assert sorted(np.nonzero(row)[0].tolist()) == sorted(samples) and set(row[sorted(samples)].tolist()) == {3}
    d1.close()
    d2.close()


def _shape_file(S, O, shape, td):
    """the file the oracle reads for a shape: the one-thread reference build where the reference is built, else synth.write_db"""
    import torch
    n, clade, L, k, f = shape
    names, lists = BC.shape_lists(shape)
    path = os.path.join(td, "want_k%d.db" % k)
    if not os.path.exists(path):
        ref = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
        if os.path.exists(ref):
            O.write_kmers_bin(os.path.join(td, "k.bin"), k, f, list(zip(names, lists)))
            O.ref_build(os.path.join(td, "k.bin"), path, 1)
        else:
            ts = [torch.from_numpy(x.view(np.int64)) for x in lists]
            pat = S.build_patterns(lambda i: ts[i], n, "cpu")
            S.write_db(path, k, f, names, pat["sample_counts"], S.to_view_arrays(pat), kmers_count=int(pat["dictionary"].numel()),
                       tables=S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k))
        O.REF_BRANCHES["test_build_handoff.py:_shape_file"] = os.path.exists(ref)
    return names, lists, path


@pytest.mark.gpu
@pytest.mark.parametrize("si", [0, 1], ids=["N48-k18", "N40-k25-f0.1"])
def test_shapes_against_the_oracle(K, S, O, dev, shape_dir, si):
    """thousands of patterns: the 256-node groups of blkbase and the 2048-node slices are crossed; with tables, against the oracle on the
    reference-built file, as test_build_upload_compare_without_a_disk does for the detour"""
    shape = BC.SHAPES[si]
    n, clade, L, k, f = shape
    names, lists, path = _shape_file(S, O, shape, shape_dir)
    d1, d2, h1, h2, hs = _both(K, lambda: K.Builder(k, f), _feed_lists(names, lists), True, dev)
    assert d2.P > (2048 if si == 0 else 256)             # (N40-k25-f0.1 keeps 1112 patterns: the 256-node groups only)
    print(hs)
    _same_handles(d1, d2, h1, h2, hs, True, [lists[i] for i in (0, 5, 17, 30, n - 1)], oracle=O.OracleDB(path))
    d1.close()
    d2.close()
    # and without tables: stage (d) is skipped, the working set of all2all is prepared at the hand-off
    d1, d2, h1, h2, hs = _both(K, lambda: K.Builder(k, f), _feed_lists(names, lists), False, dev)
    assert hs["tables_ms"] == 0 and hs["prepare_ms"] > 0 and hs["d2h_bytes"] == 0
    _same_handles(d1, d2, h1, h2, hs, False, [], oracle=O.OracleDB(path))
    d1.close()
    d2.close()


@pytest.mark.gpu
def test_protein_text_against_the_oracle(K, O, dev, golden_dir):
    """one of test_build.py's TEXT_CASES fed as text: the extractor's lists never leave the device either; the golden database holds the
    same samples in the same order, so the oracle's triangle on it is the expected one"""
    src = os.path.join(ROOT, "tests", "golden", "protein.aa_100x1000.fasta.xz")
    recs = []
    for block in lzma.open(src).read().decode().split(">")[1:]:
        head, _, body = block.partition("\n")
        recs.append((head.split(" ")[0].strip(), body.replace("\n", "").replace("\r", "")))
    gpath = os.path.join(golden_dir, "protein_aa11_diamond.db")
    g = K.HostDB(gpath, skip_hashtables=True)
    names = [r[0] for r in recs]
    assert names == g.names
    half = len(recs) // 2

    def feed(b):
        b.add_seqs(names[:half], [r[1] + "\n" for r in recs[:half]])
        b.add_seqs(names[half:], [r[1] + "\n" for r in recs[half:]])
    d1, d2, h1, h2, hs = _both(K, lambda: K.Builder(g.k, g.fraction, 0.0, K.ALPHABETS[g.alphabet]), feed, False, dev)
    assert [int(x) for x in h2.sample_kmers] == [int(x) for x in g.sample_kmers]
    _same_handles(d1, d2, h1, h2, hs, False, [], oracle=O.OracleDB(gpath))
    d1.close()
    d2.close()


@pytest.mark.gpu
def test_seeded_builder_against_the_oracle(K, O, dev, golden_dir):
    """Builder.from_db on virus_k18_part1, the genomes of part 2 added as text, handed over: the oracle on virus_k18 (the reference's build of
    both parts) gives the triangle and the rows"""
    part2 = MC.virus_entries(golden_dir, "virus.seqs.part2.list")
    texts = [b"\n".join(MC.fasta_records(os.path.join(golden_dir, e + ".fasta"))) + b"\n" for e in part2]
    names = [os.path.basename(e) for e in part2]
    seed = K.HostDB(os.path.join(golden_dir, "virus_k18_part1.db"))
    d1, d2, h1, h2, hs = _both(K, lambda: K.Builder.from_db(seed), lambda b: b.add_seqs(names, texts), True, dev)
    full = os.path.join(golden_dir, "virus_k18.db")
    assert h2.names == K.HostDB(full, skip_hashtables=True).names
    qs = [MC.oracle_words(O, texts[i].split(b"\n"), 18, "nt", 1.0) for i in (0, len(texts) - 1)]
    _same_handles(d1, d2, h1, h2, hs, True, qs, oracle=O.OracleDB(full))
    d1.close()
    d2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [False, True], ids=["all2all", "tables"])
def test_full_host_image_stores_the_same_bytes(K, S, O, dev, shape_dir, tmp_path, tables):
    """host_image=True: store() of the returned image == store() of finish(), whether or not the handle carries the tables"""
    shape = BC.SHAPES[0]
    names, lists, path = _shape_file(S, O, shape, shape_dir)
    d1, d2, h1, h2, hs = _both(K, lambda: K.Builder(shape[3], shape[4]), _feed_lists(names, lists), tables, dev, host_image=True)
    p1, p2 = str(tmp_path / "finish.db"), str(tmp_path / "handoff.db")
    h1.store(p1)
    h2.store(p2)
    assert EC.read(p1) == EC.read(p2)
    assert hs["host_image"] == 1 and hs["d2h_bytes"] > 0 and hs["copy_back_ms"] > 0 and hs["tables_ms"] > 0
    _same_handles(d1, d2, h1, h2, hs, tables, [lists[0], lists[-1]])
    d1.close()
    d2.close()


@pytest.mark.gpu
def test_refusals_and_the_end_of_the_builder(K, dev, monkeypatch):
    """statuses on valid memory: after the hand-off the builder takes nothing more and closes; another device, unknown flags and a state
    that does not fit are errors with a message, never a fault"""
    a = np.array([5, 9, 12, 40], np.uint64)
    b = K.Builder(18)
    b.add_kmers(["s0", "s1"], [a, a[:2]])
    with pytest.raises(K.KmdbError, match=r"kmdb_opts.device is 1, the builder lives on device 0"):
        b.finish_device(device=1)
    with pytest.raises(K.KmdbError, match="kmdb_db_upload: unknown bits in kmdb_opts.flags"):
        b.finish_device(flags=1 << 9)
    b.add_kmers(["s2"], [a])                                          # those refusals left the builder as it was
    d, h = b.finish_device()
    assert (d.N, h.names) == (3, ["s0", "s1", "s2"]) and d.all2all_dense().tolist() == [2, 4, 2]
    with pytest.raises(K.KmdbError, match="finished"):
        b.add_kmers(["late"], [a])
    with pytest.raises(K.KmdbError, match="finished"):
        b.finish()
    with pytest.raises(K.KmdbError, match="finished"):
        b.finish_device()
    b.close()
    d.close()
    assert K.Builder(18).handoff_stats()["total_ms"] == 0             # zeros on a builder that was not handed over
    # a limit the adds fit under and the tables of k = 25 (2^18 buckets of 16 slots at least: 32 MB) do not: the error names the bytes, the
    # builder is dead
    monkeypatch.setenv("KMDB_BUILD_DEVICE_BYTES", str(8 << 20))
    b = K.Builder(25)
    monkeypatch.delenv("KMDB_BUILD_DEVICE_BYTES")
    b.add_kmers(["m0", "m1"], [a, a[1:]])
    assert b.stats()["peak_device_bytes"] <= 8 << 20
    with pytest.raises(K.KmdbError, match=r"does not fit the device: \d+ bytes needed for"):
        b.finish_device(with_hashtables=True)
    with pytest.raises(K.KmdbError, match="dead"):
        b.finish()
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, front-end: <output> holds byte for byte what `build S <list> T.db` followed by `<mode> A T.db <output>` writes
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fe(dev, golden_dir, tmp_path):
    """(root with the virus genomes linked: the list entries resolve with cwd = root; golden path of a name; temp path of a name)"""
    root = MC.link_virus_data(golden_dir, str(tmp_path))
    return root, (lambda n: os.path.join(golden_dir, n)), (lambda n: str(tmp_path / n))


@pytest.mark.gpu
def test_front_end_dense_tables(fe):
    root, g, t = fe
    r = _cli("all2all", "-from-samples", "-k", "18", g("virus.seqs.list"), t("v.csv"), cwd=root)
    for line in ("All versus all comparison", "Building database (from fasta genomes)", "Processing samples...", "EXECUTION TIMES", "Database handed to the engine in"):
        assert line in r.stderr, line
    assert "Loading k-mer database" not in r.stderr and "Serializing database" not in r.stderr
    assert EC.read(t("v.csv")) == EC.read(g("virus.k18.csv"))
    _cli("all2all", "-from-samples", "-f", "0.1", g("virus.seqs.list"), t("vf.csv"), cwd=root)
    assert EC.read(t("vf.csv")) == EC.read(g("virus.k18.frac.csv"))
    with open(t("synth.list"), "w") as f:
        f.write(g("synth.synth") + "\n")
    _cli("all2all", "-from-samples", "-multisample-fasta", "-k", "21", t("synth.list"), t("s.a2a"))
    assert EC.read(t("s.a2a")) == EC.read(g("synth.a2a"))
    # a seeded builder: part 1 from the stored database, part 2 from its genomes
    _cli("all2all", "-from-samples", "-extend-from", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("ext.csv"), cwd=root)
    assert EC.read(t("ext.csv")) == EC.read(g("virus.k18.csv"))
    # <sample>.minhash files in
    _cli("minhash", "-k", "18", "-f", "0.1", g("virus.seqs.list"), cwd=root)
    r = _cli("all2all", "-from-samples", "-from-minhash", g("virus.seqs.list"), t("vm.csv"), cwd=root)
    assert "Building database (from minhashed k-mers)" in r.stderr
    assert EC.read(t("vm.csv")) == EC.read(g("virus.k18.frac.csv"))


@pytest.mark.gpu
def test_front_end_sparse_tables(fe):
    root, g, t = fe
    _cli("all2all", "-sparse", "-from-samples", "-k", "18", g("virus.seqs.list"), t("a.csv"), cwd=root)
    assert EC.read(t("a.csv")) == EC.read(g("virus.k18.sparse.csv"))
    _cli("all2all-sp", "-from-samples", "-k", "18", g("virus.seqs.list"), t("b.csv"), cwd=root)
    assert EC.read(t("b.csv")) == EC.read(g("virus.k18.sparse.csv"))
    with open(t("synth.list"), "w") as f:
        f.write(g("synth.synth") + "\n")
    _cli("all2all-sp", "-from-samples", "-multisample-fasta", "-k", "21", "-max", "39", "-min", "num-kmers:31", t("synth.list"), t("ab.csv"))
    assert EC.read(t("ab.csv")) == EC.read(g("synth.a2a.sparse.above-below"))


@pytest.mark.gpu
def test_front_end_distance_and_sampled_rows(fe):
    """each against `build` + the mode on the built file, in the same test"""
    root, g, t = fe
    _cli("build", "-k", "18", g("virus.seqs.list"), t("T.db"), cwd=root)
    for tag, mode, sw in (("jaccard", "all2all", ("-distance", "jaccard")),
                          ("rows", "all2all-sp", ("-sample-rows", "jaccard:3")),
                          ("phylip", "all2all", ("-phylip-out", "-distance", "mash")),
                          ("two", "all2all-sp", ("-distance", "ani", "-distance", "min", "-min", "0.5"))):
        _cli(mode, *sw, t("T.db"), t(tag + ".want"))
        _cli(mode, "-from-samples", "-k", "18", *sw, g("virus.seqs.list"), t(tag + ".got"), cwd=root)
        for suffix in ((".ani", ".min") if tag == "two" else ("",)):
            want = EC.read(t(tag + ".want" + suffix))
            assert len(want) > 1000 and EC.read(t(tag + ".got" + suffix)) == want, (tag, suffix)


@pytest.mark.gpu
def test_front_end_keep_db(fe):
    root, g, t = fe
    _cli("build", "-f", "0.1", g("virus.seqs.list"), t("T.db"), cwd=root)
    r = _cli("all2all", "-from-samples", "-f", "0.1", "-keep-db", t("kept.db"), g("virus.seqs.list"), t("v.csv"), cwd=root)
    assert "Serializing database..." in r.stderr
    assert EC.read(t("kept.db")) == EC.read(t("T.db"))
    assert EC.read(t("v.csv")) == EC.read(g("virus.k18.frac.csv"))
    _cli("all2all-sp", "-from-samples", "-f", "0.1", "-keep-db", t("kept2.db"), g("virus.seqs.list"), t("s.csv"), cwd=root)
    assert EC.read(t("kept2.db")) == EC.read(t("T.db"))
    _cli("all2all-sp", t("T.db"), t("s.want"))
    assert EC.read(t("s.csv")) == EC.read(t("s.want"))
