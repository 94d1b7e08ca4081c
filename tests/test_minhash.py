"""The minhash mode: kmdbh_minhash_store / kmdbh_minhash_load (the bytes of the reference's MihashedInputFile), the stand-alone device extractor
behind kmdb_minhash_batch_seq_alphabet (csrc/minhash.hip), the front-end's `minhash` mode and `new2all` / `one2all -from-minhash`.

Expected words never come from the code under test: the reference's recorded words (tests/golden/loader_extract.npz), the oracle's
extract_seq_alphabet (pinned to the reference by tests/test_loader_conformance.py) or a live oracle/_ref/ref_extract; expected files are
assembled here with struct.pack (minhash_cases.expected_file).

The framing of a file is 24 bytes (u32 signature, u64 count | u32 k, f64 fraction, unpadded: minhashed_input_file.h:109-118) — what
struct.calcsize gives for the fields as the reference writes them."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import loader_cases as LC
import minhash_cases as MC
from conftest import ROOT, require_ref_or_skip

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
RESOURCES = os.path.join(ROOT, "kmer-db_amd", "build", "minhash.resources.txt")
CASE_IDS = ["%s-k%d" % c for c in LC.CASES]


@pytest.fixture(scope="module")
def fx():
    return LC.Fixture()


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


def _cli(*args, cwd=None, ok=True):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, cwd=cwd)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint64 and np.array_equal(g, w), "%s: sample %d: %d words, expected %d" % (what, i, g.size, w.size)


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
STORE_CASES = (("nt", 18), ("nt", 12), ("aa", 6))                   # nt; nt widened by 16 bits; protein (widened by 10)


def test_framing_is_the_reference_fields():
    assert MC.FRAMING == 24 and len(MC.expected_file([], 18, 0.01)) == 24
    assert MC.expected_file([3], 18, 0.5) == bytes.fromhex("98badcfe" "0100000000000000" "0300000000000000" "12000000" "000000000000e03f")


@pytest.mark.parametrize("case", STORE_CASES, ids=["%s-k%d" % c for c in STORE_CASES])
def test_store_writes_the_reference_bytes_and_load_reads_them_back(K, fx, case, tmp_path):
    """kmdbh_minhash_store == MihashedInputFile::store byte for byte, for sort-unique of the reference's recorded words of several texts and
    windows; kmdbh_minhash_load gives the words, k and fraction back"""
    a, k = case
    assert LC.widen(a, k) == {("nt", 18): 4, ("nt", 12): 16, ("aa", 6): 10}[case]
    n_files = 0
    for wi in (0, 1, 2, 4):
        f = LC.WINDOWS[wi][0]
        for t in (0, 6, 10, 14):
            words = LC.sort_unique(fx.words(case, wi)[t])
            p = str(tmp_path / ("w%d_t%d.minhash" % (wi, t)))
            K.minhash_store(p, words, k, f)
            assert _read(p) == MC.expected_file(words, k, f), (case, wi, t)
            got, gk, gf = K.minhash_load(p)
            assert got.dtype == np.uint64 and np.array_equal(got, words) and gk == k and gf == f
            n_files += words.size > 0
    assert n_files >= 6, "most of the files hold words"


def test_store_of_no_words_is_the_framing_alone(K, tmp_path):
    p = str(tmp_path / "empty.minhash")
    K.minhash_store(p, np.zeros(0, np.uint64), 25, 0.01)
    assert os.path.getsize(p) == MC.FRAMING and _read(p) == MC.expected_file([], 25, 0.01)
    got, k, f = K.minhash_load(p)
    assert got.size == 0 and k == 25 and f == 0.01


def test_load_refuses_damaged_files(K, fx, tmp_path):
    words = LC.sort_unique(fx.words(("nt", 18), 0)[0])
    assert words.size > 50
    good = MC.expected_file(words, 18, 1.0)
    bad = {"wrong signature": b"\x99" + good[1:],
           "cut inside the words": good[:12 + 8 * 5 + 3],
           "cut inside the trailer": good[:-5],
           "cut inside the count": good[:9],
           "empty": b"",
           "bytes behind the trailer": good + b"\0" * 8,
           "count of 2^60 over 40 bytes": struct.pack("<IQ", MC.SIGNATURE, 1 << 60) + b"\0" * 28}
    assert len(bad["count of 2^60 over 40 bytes"]) == 40
    for what, data in bad.items():
        p = str(tmp_path / "bad.minhash")
        with open(p, "wb") as f:
            f.write(data)
        with pytest.raises(K.KmdbError):
            K.minhash_load(p)
    with pytest.raises(K.KmdbError):
        K.minhash_load(str(tmp_path / "missing.minhash"))


def test_a_damaged_count_is_no_allocation(K, tmp_path):
    """a count field of 2^60 over a 40-byte file is refused from the file's size: the message names the count, not a failed allocation"""
    p = str(tmp_path / "huge.minhash")
    with open(p, "wb") as f:
        f.write(struct.pack("<IQ", MC.SIGNATURE, 1 << 60) + b"\0" * 28)
    with pytest.raises(K.KmdbError, match="count does not agree with the size"):
        K.minhash_load(p)


@pytest.fixture(scope="module")
def virus(golden_dir, O):
    """the virus genomes: list entries, and the oracle's sorted unique words per genome and (k, fraction), computed once"""
    class V:
        entries = MC.virus_entries(golden_dir)
        _words = {}

        def words(self, entry, k, f):
            key = (entry, k, f)
            if key not in self._words:
                recs = MC.fasta_records(os.path.join(golden_dir, entry + ".fasta"))
                self._words[key] = MC.oracle_words(O, recs, k, "nt", f, 0.0)
            return self._words[key]
    v = V()
    assert len(v.entries) == 165
    return v


def _check_files(root, entries, virus, k, f):
    total = 0
    for e in entries:
        want = virus.words(e, k, f)
        assert _read(os.path.join(root, e + ".minhash")) == MC.expected_file(want, k, f), (e, k, f)
        total += want.size
    return total


@pytest.mark.parametrize("opts,f", [(("-k", "18", "-f", "0.1"), 0.1), ((), 0.01), (("-f", "0.1", "-f-start", "0.5", "-t", "3"), 0.1)],
                         ids=["k18-f0.1", "defaults", "f-start-ignored"])
def test_cli_minhash_host_extract(golden_dir, virus, tmp_path, opts, f):
    """`minhash -host-extract` (no device): every <entry>.minhash next to the entry as listed == the file assembled from the oracle's words of
    that genome's records, sort-uniqued, window (f, 0) — the default f is 0.01 and k 18, and -f-start changes nothing"""
    root = MC.link_virus_data(golden_dir, str(tmp_path))
    r = _cli("minhash", "-host-extract", *opts, os.path.join(golden_dir, "virus.seqs.list"), cwd=root)
    assert "failed:" not in r.stderr
    total = _check_files(root, virus.entries, virus, 18, f)
    assert total > 1000 * (10 if f == 0.1 else 1)


def test_cli_minhash_single_fasta_and_unreadable_entries(golden_dir, virus, tmp_path):
    """an argument that ends in a FASTA extension is ONE sample (LoaderEx::configure); an unreadable list entry is reported and skipped"""
    root = MC.link_virus_data(golden_dir, str(tmp_path))
    e = virus.entries[3]
    _cli("minhash", "-host-extract", "-f", "0.1", e + ".fasta", cwd=root)
    assert _read(os.path.join(root, e + ".fasta.minhash")) == MC.expected_file(virus.words(e, 18, 0.1), 18, 0.1)
    lst = str(tmp_path / "some.list")
    with open(lst, "w") as fh:
        fh.write("%s\n./test/virus/data/NO_SUCH_GENOME\n%s\n" % (virus.entries[0], virus.entries[1]))
    r = _cli("minhash", "-host-extract", "-f", "0.1", lst, cwd=root)
    assert "failed:./test/virus/data/NO_SUCH_GENOME" in r.stderr
    _check_files(root, virus.entries[:2], virus, 18, 0.1)
    assert not os.path.exists(os.path.join(root, "test/virus/data/NO_SUCH_GENOME.minhash"))


def test_cli_refusals(golden_dir, tmp_path):
    root = MC.link_virus_data(golden_dir, str(tmp_path))
    lst = os.path.join(golden_dir, "virus.seqs.list")
    db = os.path.join(golden_dir, "virus_k18.db")
    out = str(tmp_path / "o.csv")
    for args, word in ((("minhash", "-host-extract", "-multisample-fasta", lst), "multisample"),
                       (("minhash", "-host-extract", "-from-kmers", lst), "KMC"),
                       (("minhash", "-host-extract", "-alphabet", "aa", "-preserve-strand", lst), "preserve-strand"),
                       (("minhash", "-host-extract", "-k", "32", lst), "k-mer length"),
                       (("new2all", "-from-kmers", db, lst, out), "KMC"),
                       (("one2all", "-from-kmers", db, "x", out), "KMC")):
        r = _cli(*args, cwd=root, ok=False)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
    assert not [fn for fn in os.listdir(os.path.join(root, "test/virus/data")) if fn.endswith(".minhash")]
    r = _cli("new2all", "-from-minhash", "-multisample-fasta", db, lst, out, cwd=root, ok=False)
    assert r.returncode != 0 and "USAGE" in r.stderr
    r = _cli(ok=True)
    assert "minhash" in r.stderr and "-from-minhash" in r.stderr


def test_batch_arguments_are_checked_before_any_device_work(K):
    """k against the alphabet (alphabet.h:37), with the message of the sequence entry of new2all; an unknown alphabet"""
    for k, a, top in ((32, "nt", 31), (0, "nt", 31), (12, "aa", 11), (21, "aa6_dayhoff", 20)):
        with pytest.raises(K.KmdbError, match=r"k-mer length must be 1\.\.%d for this alphabet" % top):
            K.minhash_batch([b"ACGT"], k, a)
    with pytest.raises(K.KmdbError, match="unknown alphabet"):
        K.minhash_batch([b"ACGT"], 5, 9)
    assert K.ABI_VERSION == 8 and "#define KMDB_HAS_MINHASH 1" in open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    assert {"kmdb_minhash_batch_seq_alphabet", "kmdb_kmer_lists_free", "kmdb_minhash_geometry", "kmdbh_minhash_store", "kmdbh_minhash_load",
            "kmdbh_minhash_free"} <= set(K.capi.EXPORTS)


def test_extraction_kernels_need_no_scratch():
    """build/minhash.resources.txt (the compiler's resource remarks of the same compile): both instantiations of the extraction kernel — the
    counting pass and the writing pass — with a scratch size of 0 and no spilled register"""
    if not os.path.isdir(os.path.dirname(RESOURCES)):
        pytest.skip("the build directory %s is absent" % os.path.dirname(RESOURCES))
    assert os.path.exists(RESOURCES), "%s is missing: the build writes it for every .hip source" % RESOURCES
    found, cur = {}, None
    with open(RESOURCES, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.match(r"_ZN12_GLOBAL__N_1\d+(mh_extract_kernel)ILb([01])EE", m.group(1))
                cur = found.setdefault((k.group(1), int(k.group(2))), {}) if k else None
                continue
            m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
    assert set(found) == {("mh_extract_kernel", 0), ("mh_extract_kernel", 1)}, sorted(found)
    for key, r in found.items():
        print(key, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (key, r)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", LC.CASES, ids=CASE_IDS)
def test_device_extractor_equals_the_reference(K, fx, dev, case):
    """every case of the fixture x every window: the 15 edge texts as 15 samples of ONE batch == sort-unique of the reference's recorded words
    per text — the three windows that end at 1 (nothing kept) and the texts of length k - 1, k, k + 1 included"""
    a, k = case
    texts = fx.texts(case)
    for wi, (f, s) in enumerate(LC.WINDOWS):
        want = [LC.sort_unique(w) for w in fx.words(case, wi)]
        got = K.minhash_batch(texts, k, a, f, s, device=dev)
        _same_lists(got, want, "%s window %s" % (case, (f, s)))
        if wi in LC.TOP_WINDOWS:
            assert not any(g.size for g in got)
        st = K.minhash_stats()
        assert st["unique"] == sum(w.size for w in want) and st["kept"] >= st["unique"] and st["pieces"] == 1


EDGE_CASES = (("nt", 16), ("nt", 31), ("aa6_dayhoff", 12))
EDGE_WINDOWS = ((1.0, 0.0), (0.2, 0.4))


@pytest.mark.gpu
@pytest.mark.parametrize("window", EDGE_WINDOWS, ids=["f1", "f0.2-s0.4"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=["%s-k%d" % c for c in EDGE_CASES])
def test_run_and_tile_edges(K, O, dev, case, window):
    """one batch with every edge of the extractor's geometry (minhash_cases.edge_batch: sample lengths around R and T, invalid symbols and record
    boundaries on run and tile edges, sample boundaries inside a run and on a tile edge, tiles that keep nothing, empty samples) == the oracle"""
    a, k = case
    f, s = window
    R, T = K.minhash_geometry()
    assert R in (8, 16) and T == 256 * R
    quiet = MC.dropped_homopolymer(O, a, k, *EDGE_WINDOWS[1])
    texts, notes = MC.edge_batch(a, k, R, T, quiet)
    assert {len(t) for t in texts} >= {0, k - 1, R - 1, R, R + 1, T - 1, T, T + 1, T + k - 1}
    want = [MC.sample_words(O, t, k, a, f, s) for t in texts]
    got = K.minhash_batch(texts, k, a, f, s, device=dev)
    for g, w, note in zip(got, want, notes):
        assert np.array_equal(g, w), (note, g.size, w.size)
    by_note = {n[0]: w for n, w in zip(notes, want)}
    assert by_note["homopolymer over whole tiles"].size == (1 if f >= 1 else 0) and by_note["no symbol of the alphabet over a whole tile"].size == 0
    assert by_note["length T+k-1"].size > (T // 2 if f >= 1 else T // 20)
    st = K.minhash_stats()
    print("bases", st["bases"], "kept", st["kept"], "unique", st["unique"], "device bytes per base %.2f" % (st["scratch_bytes"] / max(1, st["bases"])))
    assert K.minhash_batch([], k, a, f, s, device=dev) == []
    assert [g.size for g in K.minhash_batch([b"", b""], k, a, f, s, device=dev)] == [0, 0]


@pytest.mark.gpu
def test_edge_batch_against_the_live_reference(K, O, dev):
    """the same batch decided by the reference's own extractor where its build travelled (skipped without it, FAILED under KMDB_REQUIRE_REF=1)"""
    require_ref_or_skip(O.REF_EXTRACT, "oracle/_ref/ref_extract (the reference's own extractor) is not built")
    assert O.have_ref_extract()
    a, k = "nt", 16
    R, T = K.minhash_geometry()
    texts, _ = MC.edge_batch(a, k, R, T, MC.dropped_homopolymer(O, a, k, *EDGE_WINDOWS[1]))
    for f, s in EDGE_WINDOWS:
        want = []
        for t in texts:
            recs = [r for r in t.split(b"\n") if r]
            want.append(LC.sort_unique(np.concatenate(O.ref_extract(a, k, f, s, recs) + [np.zeros(0, np.uint64)])))
        _same_lists(K.minhash_batch(texts, k, a, f, s, device=dev), want, "live reference, window %s" % ((f, s),))


@pytest.mark.gpu
def test_sort_and_unique(K, O, dev):
    """the same text as two samples gives two equal lists; a text and its reverse complement (nt) give equal lists; a sample of one word repeated
    3 T times gives one word"""
    R, T = K.minhash_geometry()
    rng = np.random.default_rng(20261018)
    k = 18
    t = LC.random_text(rng, "nt", 3 * T + 7, invalid_rate=0.001, lower_rate=0.2)
    rc = t[::-1].translate(bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa"))
    unit = LC.random_text(rng, "nt", k)
    repeated = (unit + b"N") * (3 * T)
    for f, s in ((1.0, 0.0), (0.5, 0.0)):
        want = MC.sample_words(O, t, k, "nt", f, s)
        got = K.minhash_batch([t, b"", t, rc, repeated], k, "nt", f, s, device=dev)
        assert want.size > T // 4 and np.array_equal(got[0], want) and np.array_equal(got[2], want) and np.array_equal(got[3], want) and got[1].size == 0
        assert np.array_equal(got[4], MC.sample_words(O, unit, k, "nt", f, s)) and got[4].size <= 1
    assert K.minhash_batch([repeated], k, "nt", 1.0, 0.0, device=dev)[0].size == 1
    st = K.minhash_stats()
    assert st["kept"] == 3 * T and st["unique"] == 1


@pytest.mark.gpu
def test_pieces(K, O, dev, monkeypatch):
    """a batch cut into three pieces (KMDB_MINHASH_BASES_PER_PIECE) gives the result of one piece; a sample longer than the budget goes alone"""
    rng = np.random.default_rng(7)
    texts = [LC.random_text(rng, "nt", n, invalid_rate=0.002) for n in (1000, 900, 1000, 0, 950, 1000, 5000, 30)]
    want = [MC.sample_words(O, t, 20, "nt", 0.3, 0.1) for t in texts]
    one = K.minhash_batch(texts[:6], 20, "nt", 0.3, 0.1, device=dev)
    assert K.minhash_stats()["pieces"] == 1
    _same_lists(one, want[:6], "one piece")
    monkeypatch.setenv("KMDB_MINHASH_BASES_PER_PIECE", "2100")
    three = K.minhash_batch(texts[:6], 20, "nt", 0.3, 0.1, device=dev)
    assert K.minhash_stats()["pieces"] == 3
    _same_lists(three, want[:6], "three pieces")
    _same_lists(K.minhash_batch(texts, 20, "nt", 0.3, 0.1, device=dev), want, "a sample beyond the budget")
    assert K.minhash_stats()["pieces"] == 5


@pytest.mark.gpu
def test_cli_minhash_on_the_device_and_from_minhash_queries(golden_dir, virus, dev, tmp_path):
    """`minhash` on the device == the Python-assembled files of the oracle's words (-f 1 and -f 0.1); `new2all -from-minhash` (dense, -sparse,
    -gpus 2) and `one2all -from-minhash` over such files reproduce the reference's goldens byte for byte"""
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    root = MC.link_virus_data(golden_dir, t("f01"))
    _cli("minhash", "-k", "18", "-f", "0.1", g("virus.seqs.list"), cwd=root)
    _check_files(root, virus.entries, virus, 18, 0.1)
    root = MC.link_virus_data(golden_dir, t("f1"))
    r = _cli("minhash", "-k", "18", "-f", "1", g("virus.seqs.list"), cwd=root)
    assert "failed:" not in r.stderr
    _check_files(root, virus.entries, virus, 18, 1.0)
    # the lists and databases of the existing golden test (test_gpu_parity.test_cli_byte_identical_to_reference_goldens), so the row names agree
    for opts, db, lst, golden in (((), "virus_k18_part1.db", "virus.seqs.part2.list", "virus.k18.n2a.csv"),
                                  (("-sparse",), "virus_k18_part1.db", "virus.seqs.part2.list", "virus.k18.n2a.sparse.csv"),
                                  (("-gpus", "2"), "virus_k18_part1.db", "virus.seqs.part2.list", "virus.k18.n2a.csv"),
                                  (("-sparse", "-gpus", "2"), "virus_k18_part1.db", "virus.seqs.part2.list", "virus.k18.n2a.sparse.csv"),
                                  ((), "virus_k18.db", "virus.seqs.list", "virus.k18.n2a.itself.csv")):
        out = t("n2a%s.csv" % "".join(opts))
        _cli("new2all", "-from-minhash", *opts, g(db), g(lst), out, cwd=root)
        assert _read(out) == _read(g(golden)), (opts, db)
    # an entry without its file is reported and skipped
    with open(t("short.list"), "w") as fh:
        fh.write("./test/virus/data/NO_SUCH_GENOME\n%s\n" % virus.entries[0])
    r = _cli("new2all", "-from-minhash", g("virus_k18.db"), t("short.list"), t("short.csv"), cwd=root)
    assert "failed:./test/virus/data/NO_SUCH_GENOME" in r.stderr and len(_read(t("short.csv")).splitlines()) == 3
    # one2all: the golden's database is k = 25, f = 0.1 (main.yml:156-160): the sample is minhashed with the database's k and -f first
    with open(t("one.list"), "w") as fh:
        fh.write("./test/virus/data/MT159713\n")
    root = MC.link_virus_data(golden_dir, t("k25"))
    _cli("minhash", "-k", "25", "-f", "0.1", t("one.list"), cwd=root)
    for opts in ((), ("-gpus", "2")):
        _cli("one2all", "-from-minhash", *opts, g("virus_k25_f01_part1.db"), "./test/virus/data/MT159713", t("MT159713.csv"), cwd=root)
        assert _read(t("MT159713.csv")) == _read(g("virus.MT159713.csv"))
    # a k = 20 file against the k = 18 database; a sample without a file
    root = MC.link_virus_data(golden_dir, t("k20"))
    _cli("minhash", "-k", "20", "-f", "1", t("one.list"), cwd=root)
    r = _cli("one2all", "-from-minhash", g("virus_k18.db"), "./test/virus/data/MT159713", t("x.csv"), cwd=root, ok=False)
    assert r.returncode != 0 and "Sample and database k-mer length differ" in r.stderr
    r = _cli("one2all", "-from-minhash", g("virus_k18.db"), "./test/virus/data/NO_SUCH_GENOME", t("x.csv"), cwd=root, ok=False)
    assert r.returncode != 0 and "Cannot open sample file: ./test/virus/data/NO_SUCH_GENOME" in r.stderr
