"""The query loaders against the reference's OWN k-mer extractor.

new2all / one2all turn sequence text into k-mer words in three places — the oracle (kmo_extract_kmers_alphabet), the host loader
(kmdbh_extract_kmers[_alphabet]) and the device loader (kmdb_new2all_batch_seq_alphabet: n2a_extract_kernel and the sort / unique / offset
kernels behind it) — all restated from one reading of the reference's kmer_extract.h and filter.h.  Here all three are compared, exactly, with
the words of the reference's own KmerHelper::extract + MinHashFilter (oracle/_ref/ref_extract, the reference's headers under the reference's
build flags): always with the words recorded in tests/golden/loader_extract.npz, and with a live run where the binary is present.
tests/loader_cases.py holds the table: both nt alphabets at k = 1 .. 31 around every widening step, every protein alphabet, seven hash windows
(fraction, start) of which three end at 1, and texts with both cases, U, letters outside the alphabet at the window edges, homopolymers, a
reverse-complement palindrome and the lengths k-1, k, k+1.

A window whose end reaches 1 keeps NOTHING: the upper threshold 2^64 does not fit 64 bits, and the reference as its own flags compile it gets
0.  kmdbh_minhash_window writes that out; the device loader, which computed the bound in hipcc-compiled code (2^63 there), takes it
from the host now."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import loader_cases as LC
from conftest import ROOT, require_ref_or_skip

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
CASE_IDS = ["%s-k%d" % c for c in LC.CASES]
GPU_IDS = ["%s-k%d" % c for c in LC.GPU_CASES]


@pytest.fixture(scope="module")
def fx():
    return LC.Fixture()


@pytest.fixture(scope="module")
def S(K):
    return importlib.import_module("kmerdb_amd.synth")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


def _su(words):
    return LC.sort_unique(words)


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g, np.uint64), w), "%s, text %d (%s): %d words, the reference has %d" % (
            what, i, LC.EDGE_LABELS[i] if i < len(LC.EDGE_LABELS) else "", len(g), len(w))


# ------------------------------------------------------------------------------------------------------------------------------------
# the databases of the device tests, built on the CPU (shared by the CPU check of the inputs and the GPU tests)
# ------------------------------------------------------------------------------------------------------------------------------------
class _Dbs:
    def __init__(self, S, golden_dir, tmp):
        self.S, self.golden_dir, self.tmp, self.made = S, golden_dir, tmp, {}

    def path(self, case, wi):
        """nt / nt-preserve: synth's database of the collection of loader_cases at the SAME window as the queries; protein: the fixture database
        (fraction 1: the queries' window thins the query side alone)"""
        a, k = case
        if not a.startswith("nt"):
            return os.path.join(self.golden_dir, "loader_%s_k%d.db" % (a, k))
        if (case, wi) not in self.made:
            S = self.S
            f, s = LC.WINDOWS[wi]
            g, pat = S.synth_database(LC.GPU_N, LC.GPU_CLADE, LC.GPU_L, k=k, fraction=f, seed=LC.GPU_SEED, start_fraction=s, preserve_strand=a == "nt-preserve")
            arr = S.to_view_arrays(pat)
            tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
            p = os.path.join(self.tmp, "%s_k%d_w%d.db" % (a, k, wi))
            S.write_db(p, k, f, [g.name(i) for i in range(LC.GPU_N)], pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables,
                       start_fraction=s, alphabet=LC.ALPHABETS.index(a))
            self.made[case, wi] = p
        return self.made[case, wi]


@pytest.fixture(scope="module")
def dbs(S, golden_dir, tmp_path_factory):
    return _Dbs(S, golden_dir, str(tmp_path_factory.mktemp("loader_dbs")))


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_texts_are_the_tables(fx):
    """the texts recorded in the fixture are the ones tests/loader_cases.py makes today (a changed generator needs a regenerated fixture), every
    case of the table is there, and the table is the one the tests were specified with"""
    assert [k for a, k in LC.CASES if a == "nt"] == [1, 4, 12, 15, 16, 17, 18, 19, 20, 22, 25, 28, 31] == [k for a, k in LC.CASES if a == "nt-preserve"]
    assert {a: [k for b, k in LC.CASES if b == a] for a in LC.PROTEIN} == {"aa": [1, 3, 8, 11, 6], "aa11_diamond": [1, 3, 10, 15], "aa12_mmseqs": [1, 3, 10, 15],
                                                                           "aa6_dayhoff": [1, 3, 14, 20, 12]}
    assert [(LC.bits(a) * k, LC.widen(a, k)) for a, k in LC.GPU_PROTEIN] == [(30, 10), (36, 4), (40, 0)]
    for case in LC.CASES:
        assert fx.texts(case) == LC.edge_texts(*case), case
        a, k = case
        t = fx.texts(case)
        assert [len(x) for x in t[11:14]] == [k - 1, k, k + 1] and len(t[14]) == 3 * k + 2
        assert t[0] != t[0].upper() and t[0] != t[0].lower() and (b"U" in t[0].upper()), "both cases and U in the random text"
    for case in LC.GPU_CASES:
        assert fx.pieces(case) == [t for _, _, t in LC.own_pieces(*case)], case


@pytest.mark.parametrize("case", LC.CASES, ids=CASE_IDS)
def test_oracle_and_host_loader_equal_the_reference(K, O, fx, case):
    """oracle extractor == the reference's recorded words and host loader == the same, word for word in extraction order, for every window —
    the three that end at 1 included (nothing is kept there); the nt-only entry kmdbh_extract_kmers as well"""
    a, k = case
    texts = fx.texts(case) + (fx.pieces(case) if case in LC.GPU_CASES else [])
    for wi, (f, s) in enumerate(LC.WINDOWS):
        want = fx.words(case, wi) + (fx.piece_words(case, wi) if case in LC.GPU_CASES and wi in LC.GPU_WINDOWS else [])
        tx = texts[: len(want)]
        what = "%s k=%d window %s" % (a, k, (f, s))
        _same_lists([O.extract_seq_alphabet(t, k, a, f, s) for t in tx], want, "oracle, " + what)
        _same_lists([K.extract_kmers_alphabet(t, k, a, f, s) for t in tx], want, "host loader, " + what)
        if a.startswith("nt"):
            _same_lists([K.extract_kmers(t, k, f, s, a == "nt-preserve") for t in tx], want, "kmdbh_extract_kmers, " + what)
        if wi in LC.TOP_WINDOWS:
            assert not any(w.size for w in want), "the reference build keeps nothing in a window that ends at 1"
    full = fx.words(case, 0)
    assert sum(w.size for w in full) >= 60, "the unfiltered window of a case holds words"
    assert full[12].size == 1 and full[11].size == 0 and full[13].size == 2, "lengths k-1, k, k+1 give 0, 1 and 2 windows"
    rep = full[14]
    assert rep.size == 3 and rep[0] == rep[2] != rep[1], "the interleaved repeat: a word, another, the first again"
    assert (int(rep[0]) ^ int(rep[1])) >> (LC.bits(a) * k) != 0 or LC.widen(a, k) == 0, "the two differ above bit bits * k wherever the word is widened"
    if LC.bits(a) <= LC.widen(a, k) <= LC.bits(a) * (k - 1):        # (a wider tail repeats the first symbol in the low bits: k = 1, 3, 4)
        assert (int(rep[0]) ^ int(rep[1])) & ((1 << (LC.bits(a) * k)) - 1) == 0, "and nowhere below it where the widening covers a symbol"


def test_hash_window_is_the_reference_builds(K, S, fx):
    """kmdbh_minhash_window (and synth's restatement of it) == the thresholds the reference's MinHashFilter object held, for every window with a
    filter (fraction < 1; at fraction 1 the reference installs a NullFilter and no loader filters); and those thresholds explain the recorded
    words: the unfiltered words whose hash (numpy restatement) lies in [lo, hi) are exactly the recorded words of the window."""
    for wi, (f, s) in enumerate(LC.WINDOWS):
        if f >= 1.0:
            continue
        want = (int(fx.window_lo[wi]), int(fx.window_hi[wi]))
        assert K.capi.minhash_window(f, s) == want, (f, s)
        assert S.minhash_window(f, s) == want, (f, s)
        assert (want[1] == 0) == (wi in LC.TOP_WINDOWS)
        lo, hi = np.uint64(want[0]), np.uint64(want[1])
        for case in LC.CASES:
            for t, (allw, kept) in enumerate(zip(fx.words(case, 0), fx.words(case, wi))):
                h = LC.minhash(allw, case[1])
                assert np.array_equal(allw[(h >= lo) & (h < hi)], kept), (case, (f, s), t)
    assert K.capi.minhash_window(0.5, 0.8)[1] == 0 and K.capi.minhash_window(0.3, 0.2) == (int(2.0 ** 64 * 0.2), int(2.0 ** 64 * 0.5))
    assert "kmdbh_minhash_window(" in open(os.path.join(ROOT, "include", "kmdb_amd.h")).read() and "kmdbh_minhash_window" in K.capi.EXPORTS
    assert K.ABI_VERSION == 8


def test_live_reference_equals_the_fixture(O, fx):
    """where the reference's sources are present `make -C oracle` builds oracle/_ref/ref_extract; the live binary gives the recorded words and
    thresholds for the whole table (skipped without the binary, FAILED under KMDB_REQUIRE_REF=1)"""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    ref = re.search(r"^REF \?= (\S+)", mk, re.M).group(1)
    if os.path.exists(os.path.join(ref, "src", "kmer_extract.h")):
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/ref_extract"], capture_output=True, text=True)
        assert r.returncode == 0 and os.path.exists(O.REF_EXTRACT), r.stderr[-2000:]
    require_ref_or_skip(O.REF_EXTRACT, "oracle/_ref/ref_extract (the reference's own extractor) is not built")
    assert O.have_ref_extract()
    for wi, (f, s) in enumerate(LC.WINDOWS):
        assert O.ref_window(f, s) == (int(fx.window_lo[wi]), int(fx.window_hi[wi])), (f, s)
        for case in LC.CASES:
            _same_lists(O.ref_extract(case[0], case[1], f, s, fx.texts(case)), fx.words(case, wi), "live reference, %s window %s" % (case, (f, s)))
    for case in LC.GPU_CASES:
        for wi in LC.GPU_WINDOWS:
            got = O.ref_extract(case[0], case[1], LC.WINDOWS[wi][0], LC.WINDOWS[wi][1], fx.pieces(case))
            assert all(np.array_equal(g, w) for g, w in zip(got, fx.piece_words(case, wi))), (case, wi)


@pytest.mark.parametrize("alphabet", ["nt", "nt-preserve"])
def test_synth_kmers_equal_the_host_loader(K, S, alphabet):
    """synth.kmers_of(..., start_fraction) == sort-unique of the host loader's words of the same genome, for every window and the k of the
    device tests (the host loader is pinned to the reference above)"""
    import torch
    gen = LC.genome_texts(alphabet)
    lut = np.full(256, 255, np.uint8)
    lut[list(b"ACGT")] = np.arange(4, dtype=np.uint8)
    for k in sorted({k for a, k in LC.GPU_CASES if a == alphabet} | {1, 31}):
        for f, s in LC.WINDOWS:
            for i in (0, 17):
                got = S.kmers_of(torch.from_numpy(lut[np.frombuffer(gen[i], np.uint8)]), k, f, s, preserve_strand=alphabet == "nt-preserve")
                want = _su(K.extract_kmers(gen[i], k, f, s, alphabet == "nt-preserve"))
                assert np.array_equal(got.numpy().view(np.uint64), want), (k, f, s, i)


def test_write_db_start_fraction_round_trip(K, O, S, tmp_path):
    """write_db / write_db_fast(start_fraction=0.4): the header field the reference writes (prefix_kmer_db.cpp:454) is read back by the front-end's
    reader (kmdbh_db_start_fraction) and by the oracle's; synth_database derives the samples in that window"""
    k, f, s = 18, 0.2, 0.4
    g, pat = S.synth_database(20, 5, 2000, k=k, fraction=f, seed=3, start_fraction=s)
    arr = S.to_view_arrays(pat)
    names = [g.name(i) for i in range(20)]
    tables = S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k)
    p1, p2 = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    S.write_db(p1, k, f, names, pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), tables=tables, start_fraction=s)
    S.write_db_fast(p2, k, f, names, pat["sample_counts"], arr, kmers_count=int(pat["dictionary"].numel()), start_fraction=s)
    for p in (p1, p2):
        h, o = K.HostDB(p, skip_hashtables=p == p2), O.OracleDB(p, skip_hashtables=p == p2)
        assert h.start_fraction == s == o.start_fraction and h.fraction == f == o.fraction and h.k == k == o.k and h.alphabet == 0
        assert [int(c) for c in o.sample_kmers] == pat["sample_counts"]
    lut = np.frombuffer(b"ACGT", np.uint8)
    want = _su(K.extract_kmers(lut[g.sample(7).numpy()].tobytes(), k, f, s))
    assert pat["sample_counts"][7] == want.size > 100
    assert np.array_equal(O.OracleDB(p1).one2all(want)[7], want.size)
    S.write_db(p1, k, 1.0, names, pat["sample_counts"], arr)                      # the default stays 0
    assert K.HostDB(p1, skip_hashtables=True).start_fraction == 0.0


def _expected_rows(O, path, words):
    o = O.OracleDB(path)
    uq = [_su(w) for w in words]
    return uq, np.stack([o.one2all(u) for u in uq])


@pytest.mark.parametrize("case", LC.GPU_CASES, ids=GPU_IDS)
def test_device_batches_are_decided_by_the_reference_alone(O, fx, dbs, case):
    """the inputs of the device tests, checked on the CPU with the reference's words and the oracle's one2all alone: in every non-empty window
    at least 8 of the 24 rows are non-zero and a clean own piece finds ALL its k-mers in its own sample; in the window (0.7, 0.3) the reference
    keeps no k-mer of any query and synth's database is empty"""
    texts, words, meta = LC.gpu_batch(fx, case)
    assert len(texts) == 24
    for wi in LC.GPU_WINDOWS:
        path = dbs.path(case, wi)
        uq, rows = _expected_rows(O, path, words[wi])
        if wi in LC.TOP_WINDOWS:
            assert not any(u.size for u in uq) and not rows.any()
            if case[0].startswith("nt"):
                assert int(O.OracleDB(path).sample_kmers.sum()) == 0
            continue
        assert int((rows.sum(1) > 0).sum()) >= 8, (case, wi)
        for q, (sample, clean) in enumerate(meta):
            if clean:
                assert uq[q].size > 0 and rows[q, sample] == uq[q].size, (case, wi, q)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wi", LC.GPU_WINDOWS, ids=["f1", "f0.2-s0.4", "f0.7-s0.3"])
@pytest.mark.parametrize("case", LC.GPU_CASES, ids=GPU_IDS)
def test_device_loader_equals_the_reference(K, O, fx, dbs, dev, case, wi):
    """kmdb_new2all_batch_seq_alphabet on 24 queries (own pieces, noisy own pieces, the edge texts) against a database of 48 samples built at the
    queries' window: out_kmer_counts == the sizes of sort-unique of the reference's words, the rows == the oracle's one2all of those words ==
    kmdb_new2all_batch of the host loader's words; a clean own piece has its unique count in its own column; in (0.7, 0.3), the top window as
    the reference build has it, every count is 0.  k = 12 .. 22 (widening 16 .. 0, sort width 40 .. 44 bits) keeps the bucket counts <= 4096;
    k >= 26 needs >= 2^20 hash tables per database and is left to the CPU tests above."""
    a, k = case
    f, s = LC.WINDOWS[wi]
    texts, words, meta = LC.gpu_batch(fx, case)
    path = dbs.path(case, wi)
    h = K.HostDB(path)
    assert K.ALPHABETS[h.alphabet] == a and h.k == k and len(h.view_arrays()["bucket_offset"]) - 1 <= 4096
    d = K.DeviceDB(h, device=dev, with_hashtables=True)
    got, cnt = d.new2all_seq(texts, fraction=f, start_fraction=s, alphabet=h.alphabet)
    uq, rows = _expected_rows(O, path, words[wi])
    print("counts", [int(c) for c in cnt], "reference", [u.size for u in uq])
    assert [int(c) for c in cnt] == [u.size for u in uq]
    assert np.array_equal(got, rows)
    host = [K.sort_unique(K.extract_kmers_alphabet(t, k, a, f, s)) for t in texts]
    assert np.array_equal(d.new2all(host), got)
    if wi in LC.TOP_WINDOWS:
        assert not cnt.any() and not got.any()
    else:
        assert int((got.sum(1) > 0).sum()) >= 8
        for q, (sample, clean) in enumerate(meta):
            if clean:
                assert got[q, sample] == cnt[q] > 0
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 20])
def test_sequence_queries_on_query_shards(K, O, fx, dbs, dev, k):
    """three kmdb_db_upload_query_shard handles on the one device, at widening 8 (k = 16) and 0 (k = 20): a shard keeps the positions whose word
    it owns (word >> 32, widening included); the rows ADDED into one device buffer equal the unsharded rows and the reference's, and the
    per-shard counts add up to the query's unique count"""
    import torch
    case = ("nt", k)
    texts, words, _ = LC.gpu_batch(fx, case)
    for wi in (0, 2):
        f, s = LC.WINDOWS[wi]
        path = dbs.path(case, wi)
        h = K.HostDB(path)
        uq, rows = _expected_rows(O, path, words[wi])
        whole = K.DeviceDB(h, device=dev, with_hashtables=True)
        exp, cnt = whole.new2all_seq(texts, fraction=f, start_fraction=s)
        whole.close()
        assert np.array_equal(exp, rows) and [int(c) for c in cnt] == [u.size for u in uq]
        buf = torch.zeros((len(texts), rows.shape[1]), dtype=torch.int32, device=torch.device("cuda", dev))
        total = np.zeros(len(texts), np.uint64)
        for sh in range(3):
            d = K.DeviceDB(h, device=dev, query_shard=(sh, 3))
            c = d.new2all_seq_device(texts, buf.data_ptr(), fraction=f, start_fraction=s)
            own = [int((((u >> np.uint64(32)) % np.uint64(3)) == sh).sum()) for u in uq]
            assert [int(x) for x in c] == own, (k, wi, sh)
            total += c
            d.close()
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), rows)
        assert np.array_equal(total, cnt)


def _virus_genomes(golden_dir, limit):
    with open(os.path.join(golden_dir, "virus.seqs.list")) as f:
        entries = [ln.strip() for ln in f if ln.strip()][:limit]
    out = []
    for e in entries:
        raw = open(os.path.join(golden_dir, e + ".fasta"), "rb").read()
        out.append(b"".join(raw.split(b"\n")[1:]).replace(b"\r", b"").replace(b">", b"N"))
    return out


BATCH_LENGTHS = (0, 17, 18, 19, 255, 256, 257, 2047, 2048, 2049)


def _shape_batch(golden_dir, delta):
    """600 queries with lengths of BATCH_LENGTHS — stretches of the virus genomes with lower case, U and N — runs of empty queries at the head, in
    the middle and at the tail, and a total length of a multiple of 2048 plus delta (the own-positions tile of a query shard is 2048 wide)"""
    rng = np.random.default_rng(600 + delta)
    gen = _virus_genomes(golden_dir, 8)
    lens = rng.choice(BATCH_LENGTHS, 600)
    lens[:5] = 0
    lens[300:304] = 0
    lens[-6:] = 0
    lens[5] = 2049
    lens[6] = 0
    lens[6] = (delta - int(lens.sum())) % 2048                     # one query of a length of its own brings the total to m * 2048 + delta
    assert (int(lens.sum()) - delta) % 2048 == 0
    texts = []
    for n in lens:
        g = gen[int(rng.integers(len(gen)))]
        at = int(rng.integers(0, len(g) - 2100))
        t = bytearray(g[at: at + int(n)])
        for i in np.nonzero(rng.random(len(t)) < 0.01)[0]:
            t[i] = ord("N")
        if rng.random() < 0.3:
            t = bytearray(bytes(t).lower().replace(b"t", b"u"))
        texts.append(bytes(t))
    return texts


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_batch_shapes(K, golden_dir, dev, monkeypatch, delta):
    """600 queries in one call (n2a_query_offsets_kernel over three blocks; empty queries at the head, in the middle and at the tail; lengths
    around k = 18, 256 and 2048; the total just below, at and just above a multiple of 2048) on the whole handle and on three query shards:
    counts and rows == the host loader's words through kmdb_new2all_batch.  The same batch cut into pieces of at most 1, 300 and 5000 bases
    (KMDB_N2A_BASES_PER_PIECE, read per call; a longer query goes alone) gives the same rows and counts."""
    import torch
    k = 18
    texts = _shape_batch(golden_dir, delta)
    assert len(texts) == 600 and (sum(len(t) for t in texts) - delta) % 2048 == 0 and {len(t) for t in texts} >= set(BATCH_LENGTHS)
    host = [K.sort_unique(K.extract_kmers(t, k)) for t in texts]
    h = K.HostDB(os.path.join(golden_dir, "virus_k18.db"))
    d = K.DeviceDB(h, device=dev, with_hashtables=True)
    exp = d.new2all(host)
    assert int((exp.sum(1) > 0).sum()) > 300
    monkeypatch.delenv("KMDB_N2A_BASES_PER_PIECE", raising=False)
    got, cnt = d.new2all_seq(texts)
    assert [int(c) for c in cnt] == [x.size for x in host]
    assert np.array_equal(got, exp)
    for budget in (1, 300, 5000):
        monkeypatch.setenv("KMDB_N2A_BASES_PER_PIECE", str(budget))
        g2, c2 = d.new2all_seq(texts)
        assert np.array_equal(c2, cnt) and np.array_equal(g2, exp), budget
    monkeypatch.delenv("KMDB_N2A_BASES_PER_PIECE")
    d.close()
    buf = torch.zeros((600, exp.shape[1]), dtype=torch.int32, device=torch.device("cuda", dev))
    total = np.zeros(600, np.uint64)
    for sh in range(3):
        ds = K.DeviceDB(h, device=dev, query_shard=(sh, 3))
        total += ds.new2all_seq_device(texts, buf.data_ptr())
        ds.close()
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), exp) and np.array_equal(total, cnt)


@pytest.mark.gpu
def test_front_end_passes_the_start_fraction(K, O, fx, dbs, dev, tmp_path):
    """one2all and new2all of two FASTA records against a synth database written with -f 0.2 -f-start 0.4: the front-end hands the database's
    start fraction to the loaders; the CSV equals, byte for byte, the oracle's text of the reference's words"""
    case, wi = ("nt", 16), 2
    f, s = LC.WINDOWS[wi]
    path = dbs.path(case, wi)
    o = O.OracleDB(path)
    assert o.start_fraction == s and o.fraction == f
    texts, words, _ = LC.gpu_batch(fx, case)
    recs = [("r0", texts[0], words[wi][0]), ("r1", texts[9], words[wi][9])]
    fa = tmp_path / "q.fa"
    fa.write_bytes(b"".join(b">" + n.encode() + b"\n" + t + b"\n" for n, t, _ in recs))
    # one2all: the records are one sample, named like the argument
    uq = _su(np.concatenate([w for _, _, w in recs]))
    out = tmp_path / "o2a.csv"
    r = subprocess.run([EXE, "one2all", path, str(fa), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = O.format_new2all(o.k, o.fraction, o.names, o.sample_kmers, [(str(fa), uq.size)], [o.one2all(uq)])
    assert out.read_bytes() == want[:-1] and uq.size > 10
    # new2all -multisample-fasta: every record a query
    lst = tmp_path / "q.list"
    lst.write_text(str(tmp_path / "q") + "\n")
    out = tmp_path / "n2a.csv"
    r = subprocess.run([EXE, "new2all", "-multisample-fasta", path, str(lst), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    us = [_su(w) for _, _, w in recs]
    want = O.format_new2all(o.k, o.fraction, o.names, o.sample_kmers, [(n, u.size) for (n, _, _), u in zip(recs, us)], [o.one2all(u) for u in us])
    assert out.read_bytes() == want
