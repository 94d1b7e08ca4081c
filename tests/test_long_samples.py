"""Long samples: the merge-union of two ascending lists on the device (kmdb_sorted_union_device, csrc/sorted_union.hip), the extraction of a
sample in sections joined by it (csrc/minhash.hip: KMDB_MINHASH_MAX_SAMPLE_BASES), the builder's text entry over such samples and the
front-end's minhash / build / new2all / one2all with them.

Expected results never come from the code under test: numpy.union1d; the oracle's extractor (minhash_cases.sample_words) and the host
extractor (K.extract_kmers_alphabet + K.sort_unique); the reference's golden tables."""
import os
import subprocess

import numpy as np
import pytest

import long_samples_cases as LS
import minhash_cases as MC
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


@pytest.fixture(scope="module")
def cases(K):
    """the union's inputs and numpy's unions of them, computed once"""
    R, T = K.sorted_union_geometry()
    c = LS.union_cases(T)
    return {name: (a, b, np.union1d(a, b)) for name, (a, b) in c.items()}


def _cli(*args, cwd=None, ok=True, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, cwd=cwd, env=e)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _to_device(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64)).cuda()


def _union_on_device(K, a, b, dev, slack=0):
    """(the words written, the words behind them in a buffer that was filled with a marker)"""
    import torch
    da, db = _to_device(a), _to_device(b)
    cap = a.size + b.size + slack
    out = torch.full((cap + 8,), -1, dtype=torch.int64, device="cuda")
    n = K.sorted_union_device(da.data_ptr() if a.size else None, a.size, db.data_ptr() if b.size else None, b.size, out.data_ptr(), cap, device=dev)
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint64)
    return host[:n], host[n:]


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_additive(K):
    hdr = open(os.path.join(ROOT, "include", "kmdb_amd.h")).read()
    assert K.ABI_VERSION == 8 and "#define KMDB_HAS_LONG_SAMPLES 1" in hdr
    L = K.lib()
    for name in ("kmdb_sorted_union_device", "kmdb_sorted_union_geometry", "kmdb_minhash_long_stats_get"):
        assert name in K.capi.EXPORTS and name + "(" in hdr and hasattr(L, name), name
    R, T = K.sorted_union_geometry()
    assert R >= 1 and T % R == 0 and T // R in (64, 128, 256, 512, 1024)
    assert set(K.minhash_long_stats()) >= {"long_samples", "sections", "union_words_in", "union_words_out", "union_ms", "peak_bytes"}


def test_union_refusals_come_before_any_device_work(K):
    """capacity below na + nb and a null array with a size, each under the entry's name — decided from the arguments alone"""
    with pytest.raises(K.KmdbError, match=r"^kmdb_sorted_union_device: the output holds 9 words, fewer than the 4 \+ 6"):
        K.sorted_union_device(0x1000, 4, 0x2000, 6, 0x3000, 9)
    for args in ((None, 3, 0x2000, 2, 0x3000, 5), (0x1000, 3, None, 2, 0x3000, 5), (0x1000, 3, 0x2000, 2, None, 5)):
        with pytest.raises(K.KmdbError, match=r"^kmdb_sorted_union_device: a null array with a size that is not 0"):
            K.sorted_union_device(*args)


def test_piece_counts_restated_from_the_lengths():
    """long_samples_cases.pieces_of on batches counted by hand (what the device tests compare the statistics with)"""
    assert LS.sections_of(1000, 700) == 0 and LS.sections_of(1001, 700) == 2 and LS.sections_of(1001, 4101) == 1 and LS.sections_of(1401, 700) == 3
    assert LS.pieces_of([1000, 900, 1000, 0, 950, 1000], 2100, 1 << 30) == (3, 0, 0)              # test_minhash.test_pieces
    assert LS.pieces_of([1000, 900, 1000, 0, 950, 1000, 5000, 30], 2100, 1 << 30) == (5, 0, 0)
    assert LS.pieces_of([300, 2500, 0, 800, 3000, 50], 700) == (1 + 4 + 2 + 5 + 1, 2, 9)
    assert LS.pieces_of([(1 << 31) + (1 << 20)], 512 << 20, 1 << 30) == (5, 1, 5)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the union alone
# ------------------------------------------------------------------------------------------------------------------------------------
def _case_names():
    return sorted(LS.union_cases(2048, big=100))          # (the names depend neither on the tile nor on the size of the random case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _case_names())
def test_union_equals_numpy(K, dev, cases, name):
    """A ∪ B == numpy.union1d(A, B); nothing is written behind the union's last word (capacity na + nb + 5)"""
    a, b, want = cases[name]
    got, behind = _union_on_device(K, a, b, dev, slack=5)
    assert got.size == want.size, (name, got.size, want.size)
    assert np.array_equal(got, want), (name, int(np.argmax(got != want)))
    assert bool(np.all(behind == np.uint64((1 << 64) - 1))), name
    # the sides exchanged: the same union
    got, _ = _union_on_device(K, b, a, dev)
    assert np.array_equal(got, want), name + " (sides exchanged)"


@pytest.mark.gpu
def test_union_tiles_of_the_cases(K, cases):
    """the cases are what they are named after for the tile of THIS build"""
    R, T = K.sorted_union_geometry()
    for tiles in (1, 2):
        for delta in (-1, 0, 1):
            a, b, want = cases["merged length %dT%+d" % (tiles, delta)]
            assert a.size + b.size == tiles * T + delta == want.size
    a, b, want = cases["a duplicate pair straddling both borders of three tiles"]
    assert a.size + b.size == 3 * T and want.size == 3 * T - 2
    a, b, want = cases["1e6 random words, 30 % overlap"]
    assert a.size == 1000000 and a.size + b.size - want.size == 300000


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: sections
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config", LS.CONFIGS, ids=["%s-k%d" % c for c in LS.CONFIGS])
def test_sections_equal_the_oracle(K, O, dev, monkeypatch, config):
    """texts of 1001, 2500 and 9000 bytes x budgets 700, 997, 4101 x two windows with the threshold at 1000: the words of the oracle on the whole
    text, and as many sections as the lengths give"""
    a, k = config
    monkeypatch.setenv("KMDB_MINHASH_MAX_SAMPLE_BASES", str(LS.MAX_SAMPLE))
    texts = [LS.section_text(a, k, n) for n in LS.LENGTHS]
    for f, s in LS.WINDOWS:
        want = [MC.sample_words(O, t, k, a, f, s) for t in texts]
        assert want[2].size > (30 if k == 5 or f < 1 else 4000)
        for budget in LS.BUDGETS:
            monkeypatch.setenv("KMDB_MINHASH_BASES_PER_PIECE", str(budget))
            for t, w in zip(texts, want):
                got = K.minhash_batch([t], k, a, f, s, device=dev)[0]
                assert np.array_equal(got, w), (config, f, budget, len(t), got.size, w.size)
                st, ls = K.minhash_stats(), K.minhash_long_stats()
                n_sec = LS.sections_of(len(t), budget)
                assert n_sec >= 1 and ls["sections"] == n_sec == st["pieces"] and ls["long_samples"] == 1, (budget, len(t), st, ls)
                assert st["unique"] == w.size and st["bases"] == len(t)
                assert ls["union_words_out"] <= ls["union_words_in"] and (n_sec > 1 or ls["union_words_in"] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (5, 18))
def test_crafted_cuts(K, O, dev, monkeypatch, k):
    """cuts inside a run, around an invalid byte, around a record end, k - 1 and k symbols after a record start, a last section of one symbol,
    a text without a symbol — and, with a budget of 1, a cut behind EVERY symbol"""
    budget = 700
    monkeypatch.setenv("KMDB_MINHASH_MAX_SAMPLE_BASES", str(LS.MAX_SAMPLE))
    monkeypatch.setenv("KMDB_MINHASH_BASES_PER_PIECE", str(budget))
    for what, t in LS.crafted_cuts(k, budget):
        for f, s in LS.WINDOWS:
            want = MC.sample_words(O, t, k, "nt", f, s)
            got = K.minhash_batch([t], k, "nt", f, s, device=dev)[0]
            assert np.array_equal(got, want), (what, k, f, got.size, want.size)
            assert K.minhash_long_stats()["sections"] == LS.sections_of(len(t), budget) >= 3
        if what == "only invalid bytes":
            assert want.size == 0
        if what == "one word repeated across the cuts":
            assert MC.sample_words(O, t, k, "nt", 1.0, 0.0).size <= k
    monkeypatch.setenv("KMDB_MINHASH_MAX_SAMPLE_BASES", "40")
    monkeypatch.setenv("KMDB_MINHASH_BASES_PER_PIECE", "1")
    t = LS.section_text("nt", k, 41)
    assert np.array_equal(K.minhash_batch([t], k, "nt", 1.0, 0.0, device=dev)[0], MC.sample_words(O, t, k, "nt", 1.0, 0.0))
    assert K.minhash_long_stats()["sections"] == 41


@pytest.mark.gpu
def test_a_long_sample_between_short_ones(K, O, dev, monkeypatch):
    """one batch of short and long samples: every list right, in input order; pieces and sections as the lengths give them"""
    lengths = (300, 2500, 0, 800, 3000, 50, 1000, 1001)
    k, a, f, s = 20, "nt", 0.3, 0.1
    texts = [LS.section_text(a, k, n) if n else b"" for n in lengths]
    want = [MC.sample_words(O, t, k, a, f, s) for t in texts]
    monkeypatch.setenv("KMDB_MINHASH_MAX_SAMPLE_BASES", str(LS.MAX_SAMPLE))
    for budget in (700, 2100):
        monkeypatch.setenv("KMDB_MINHASH_BASES_PER_PIECE", str(budget))
        got = K.minhash_batch(texts, k, a, f, s, device=dev)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (budget, i, lengths[i], g.size, w.size)
        pieces, longs, sections = LS.pieces_of(lengths, budget)
        st, ls = K.minhash_stats(), K.minhash_long_stats()
        assert (st["pieces"], ls["long_samples"], ls["sections"]) == (pieces, longs, sections) and longs == 3
        assert st["unique"] == sum(w.size for w in want) and st["bases"] == sum(lengths)
        assert ls["peak_bytes"] > 0 and ls["union_ms"] > 0
    # without the switch nothing is long: the statistics of a call are its own
    monkeypatch.delenv("KMDB_MINHASH_MAX_SAMPLE_BASES")
    got = K.minhash_batch(texts, k, a, f, s, device=dev)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert K.minhash_long_stats()["long_samples"] == 0 and K.minhash_long_stats()["sections"] == 0
    assert K.minhash_stats()["pieces"] == LS.pieces_of(lengths, 2100, 1 << 30)[0]


@pytest.mark.gpu
def test_the_builder_takes_long_samples(K, dev, monkeypatch, tmp_path):
    """Builder.add_seqs with samples cut into sections stores, byte for byte, the file the same genomes give through add_kmers with the host
    extractor's lists"""
    k, f, s = 18, 0.5, 0.0
    lengths = (1500, 400, 3100, 0, 2200)
    rng = np.random.default_rng(20261020)
    base = LS.section_text("nt", k, 3100)
    texts = []
    for n in lengths:                                               # relatives: shared stretches give patterns with several samples
        t = bytearray(base[:n])
        for at in rng.choice(max(n, 1), n // 50, replace=False):
            t[at] = b"ACGT"[rng.integers(4)]
        texts.append(bytes(t))
    names = ["g%d" % i for i in range(len(texts))]
    lists = [K.sort_unique(np.concatenate([K.extract_kmers_alphabet(r, k, "nt", f, s) for r in t.split(b"\n")] + [np.zeros(0, np.uint64)])) for t in texts]
    assert lists[2].size > 500
    b = K.Builder(k, f, s, "nt", device=dev)
    b.add_kmers(names, lists)
    b.finish().store(str(tmp_path / "host.db"))
    b.close()
    monkeypatch.setenv("KMDB_MINHASH_MAX_SAMPLE_BASES", str(LS.MAX_SAMPLE))
    monkeypatch.setenv("KMDB_MINHASH_BASES_PER_PIECE", "700")
    b = K.Builder(k, f, s, "nt", device=dev)
    b.add_seqs(names, texts)
    assert K.minhash_long_stats()["sections"] == LS.pieces_of(lengths, 700)[2] == 3 + 5 + 4
    st = b.stats()
    assert st["samples"] == len(names) and st["kmers_added"] == sum(x.size for x in lists)
    b.finish().store(str(tmp_path / "device.db"))
    b.close()
    assert _read(str(tmp_path / "device.db")) == _read(str(tmp_path / "host.db"))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: one real size
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_sample_beyond_two_to_the_31_bases(K, dev):
    """2^31 + 2^20 bases — a random block of 1 MiB repeated — with the default switches: not refused, at least 4 sections, and the words of two
    concatenated blocks from the host extractor (every window of the sample lies inside two neighbouring blocks)"""
    assert "KMDB_MINHASH_MAX_SAMPLE_BASES" not in os.environ and "KMDB_MINHASH_BASES_PER_PIECE" not in os.environ
    k, f = 18, 0.01
    rng = np.random.default_rng(20261020)
    block = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1 << 20)]
    want = K.sort_unique(K.extract_kmers_alphabet(np.concatenate([block, block]).tobytes(), k, "nt", f, 0.0))
    text = np.tile(block, 2049)
    assert text.size == (1 << 31) + (1 << 20)
    got = K.minhash_batch([text], k, "nt", f, 0.0, device=dev)[0]
    st, ls = K.minhash_stats(), K.minhash_long_stats()
    print(st, ls)
    assert want.size > 5000 and np.array_equal(got, want)
    assert ls["long_samples"] == 1 and ls["sections"] == st["pieces"] >= 4 and st["bases"] == text.size


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the command line
# ------------------------------------------------------------------------------------------------------------------------------------
SECTIONED = {"KMDB_MINHASH_MAX_SAMPLE_BASES": "3000", "KMDB_MINHASH_BASES_PER_PIECE": "2100", "KMDB_VERBOSE": "1"}


@pytest.mark.gpu
def test_cli_with_every_genome_in_sections(K, O, dev, golden_dir, tmp_path):
    """minhash, build + all2all, new2all and one2all with the virus genomes cut into sections of 2100 bases reproduce the files assembled from
    the oracle's words and the reference's golden tables, byte for byte"""
    g = lambda n: os.path.join(golden_dir, n)   # noqa: E731
    t = lambda n: str(tmp_path / n)             # noqa: E731
    entries = MC.virus_entries(golden_dir)
    # minhash: <entry>.minhash == MihashedInputFile::store of the oracle's words (what test_minhash._check_files expects)
    root = MC.link_virus_data(golden_dir, t("mh"))
    r = _cli("minhash", "-k", "18", "-f", "0.1", g("virus.seqs.list"), cwd=root, env=SECTIONED)
    assert "failed:" not in r.stderr and "long samples in" in r.stderr
    for e in entries:
        want = MC.oracle_words(O, MC.fasta_records(os.path.join(golden_dir, e + ".fasta")), 18, "nt", 0.1, 0.0)
        assert _read(os.path.join(root, e + ".minhash")) == MC.expected_file(want, 18, 0.1), e
    # build + all2all
    r = _cli("build", "-k", "18", g("virus.seqs.list"), t("v.db"), cwd=root, env=SECTIONED)
    assert "[kmdb] build:" in r.stderr and "long samples in" in r.stderr
    _cli("all2all", t("v.db"), t("v.csv"))
    assert _read(t("v.csv")) == _read(g("virus.k18.csv"))
    # new2all / one2all: every query is a long query, extracted by the sectioned extractor and entered as a k-mer list
    env = dict(SECTIONED, KMDB_LONG_QUERY_BASES="1000")
    r = _cli("new2all", g("virus_k18_part1.db"), g("virus.seqs.part2.list"), t("n2a.csv"), cwd=root, env=env)
    assert "[kmdb] long query:" in r.stderr
    assert _read(t("n2a.csv")) == _read(g("virus.k18.n2a.csv"))
    r = _cli("one2all", g("virus_k25_f01_part1.db"), "./test/virus/data/MT159713", t("MT159713.csv"), cwd=root, env=env)
    assert "[kmdb] long query:" in r.stderr
    assert _read(t("MT159713.csv")) == _read(g("virus.MT159713.csv"))
