"""The build mode: kmdb_build_* (csrc/build.hip), kmdbh_db_store (csrc/host_db.cpp) and `kmer-db-amd build`.

Everything is compared exactly.  The pattern section of a built file is the one-thread reference build's byte for byte once bytes 36..39
of every 40-byte pattern header are zeroed (the reference never writes them, pattern.cpp:35-37); the hashtable section is compared by
content — per bucket the set of (key, value) items — because capacities and slot positions depend on the reference's insertion history.
Inputs and the section compare live in tests/build_cases.py."""
import importlib
import lzma
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import build_cases as BC
import conftest
import minhash_cases as MC
from conftest import DBS, ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
RESOURCES = os.path.join(ROOT, "kmer-db_amd", "build", "build.resources.txt")
REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")


@pytest.fixture(scope="module")
def S(K):
    return importlib.import_module("kmerdb_amd.synth")


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _require_ref():
    return os.environ.get("KMDB_REQUIRE_REF", "") == "1"


def _cli(*args, cwd=None, ok=True):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, cwd=cwd)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def _same_sections(got, want, tables="bytes"):
    """header + samples equal, patterns equal under the section compare; tables byte for byte, or by content"""
    x, y = BC.split_db(got), BC.split_db(want)
    assert x["head"] == y["head"], "header / sample table differ"
    assert x["P"] == y["P"]
    assert BC.masked_patterns(x["patterns_raw"]) == BC.masked_patterns(y["patterns_raw"]), "pattern sections differ"
    if tables == "bytes":
        assert x["tables_raw"] == y["tables_raw"], "hashtable sections differ"
    else:
        assert x["n_buckets"] == y["n_buckets"]
        assert BC.table_sets(x["tables"]) == BC.table_sets(y["tables"]), "a bucket holds other items"
        BC.assert_tables_well_formed(x["tables"])


def _queries_bin(O, path, k, f, lists):
    O.write_kmers_bin(path, k, f, [("q%d" % i, q) for i, q in enumerate(lists)])


def _build(K, k, f, names, lists, calls=None, alphabet="nt", start=0.0):
    """add_kmers in calls of the given sizes (None: one call), finish -> HostDB"""
    b = K.Builder(k, f, start, alphabet)
    try:
        at = 0
        for n in (calls or [len(names)]):
            b.add_kmers(names[at: at + n], lists[at: at + n])
            at += n
        assert at == len(names)
        h = b.finish()
        st = b.stats()
        assert st["samples"] == len(names) and st["kmers_added"] == sum(len(x) for x in lists)
        return h, st
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem", DBS)
def test_store_round_trip(K, golden_dir, tmp_path, stem):
    """kmdbh_db_load(mode 0) -> kmdbh_db_store == the original: header, samples and tables byte for byte, patterns under the section compare
    (is_parent, which the fixtures carry from the real reference, included)"""
    src = os.path.join(golden_dir, stem + ".db")
    out = str(tmp_path / "stored.db")
    h = K.HostDB(src)
    h.store(out)
    h.close()
    got, want = _read(out), _read(src)
    assert len(got) == len(want)
    _same_sections(got, want)
    # the writer's is_parent is "some pattern names this one as its parent": the reference's own flag says the same in every fixture
    hdr = BC.pattern_headers(BC.split_db(want)["patterns_raw"])
    parents = {f[1] for f in hdr if f[1] >= 0}
    assert [f[6] & 0xff for f in hdr] == [1 if p in parents else 0 for p in range(len(hdr))]
    # a database loaded without its tables cannot be stored
    h2 = K.HostDB(src, skip_hashtables=True)
    with pytest.raises(K.KmdbError, match="no hashtables"):
        h2.store(str(tmp_path / "no.db"))


@pytest.mark.parametrize("stem", DBS)
def test_stored_file_is_read_by_the_reference(K, O, golden_dir, tmp_path, stem):
    """the reference's own reader takes the stored file: all2all and one2all return what they return for the original"""
    conftest.require_ref_or_skip(REF_DRIVER, "needs the reference build (oracle/_ref/ref_driver)")
    src = os.path.join(golden_dir, stem + ".db")
    out = str(tmp_path / "stored.db")
    h = K.HostDB(src)
    h.store(out)
    a, _ = O.ref_all2all(src, str(tmp_path / "a.u32"))
    b, _ = O.ref_all2all(out, str(tmp_path / "b.u32"))
    assert np.array_equal(a, b)
    # queries made of the database's own k-mers (every 7th item of its tables) and a few that are not in it
    v = h.view_arrays()
    slots, boff = v["slots"], v["bucket_offset"]
    bucket = np.repeat(np.arange(boff.size - 1, dtype=np.uint64), np.diff(boff).astype(np.int64))
    used = (slots >> np.uint64(32)) != np.uint64(BC.EMPTY_VAL)
    kmers = np.sort((bucket[used] << np.uint64(32)) | (slots[used] & np.uint64(0xffffffff)))
    qs = [kmers[::7], kmers[3::11], np.unique(np.concatenate([kmers[:5], kmers[:5] + np.uint64(1)]))]
    _queries_bin(O, str(tmp_path / "q.bin"), h.k, h.fraction, qs)
    ra, _ = O.ref_one2all(src, str(tmp_path / "q.bin"), str(tmp_path / "ra.u32"))
    rb, _ = O.ref_one2all(out, str(tmp_path / "q.bin"), str(tmp_path / "rb.u32"))
    assert ra.size == len(qs) * h.N and np.array_equal(ra, rb)


def test_cli_refusals_and_usage(tmp_path):
    """refused before any device is touched: exit status and message"""
    lst, db = str(tmp_path / "x.list"), str(tmp_path / "x.db")
    with open(lst, "w") as f:
        f.write("nothing\n")
    for args, word in ((("build", "-extend", lst, db), "build -extend is not supported: rebuild from the sample list"),
                       (("build", "-from-kmers", lst, db), "KMC k-mer input (-from-kmers) is not supported"),
                       (("build", "-from-kmers", "-from-minhash", lst, db), "-from-kmers and -from-minhash switches exclude one another"),
                       (("build", "-alphabet", "aa", "-preserve-strand", lst, db), "Switch -preserve-strand applies only to nt alphabet"),
                       (("build", "-alphabet", "klingon", lst, db), "Unknown alphabet"),
                       (("build", "-k", "32", lst, db), "K-mer length for the given alphabet cannot exceed 31"),
                       (("build", "-alphabet", "aa", "-k", "12", lst, db), "cannot exceed 11")):
        r = _cli(*args, ok=False)
        assert r.returncode not in (0, -11, -6) and ("ERROR: " + word if not word.startswith("cannot") else word) in r.stderr, (args, r.stderr)
        assert not os.path.exists(db)
    r = _cli("build", lst, ok=False)                                   # a missing argument
    assert r.returncode != 0 and "USAGE" in r.stderr and "kmer-db-amd build" in r.stderr
    r = _cli("build", "-k", "18", str(tmp_path / "no_such.list"), db, ok=False)
    assert r.returncode != 0 and "Unable to open input file" in r.stderr
    r = _cli()
    assert "build -from-minhash" in r.stderr and "-extend" in r.stderr


def test_build_kernels_use_no_scratch():
    """build/build.resources.txt (the compiler's resource remarks of the same compile): every kernel of build.hip with a scratch size of 0
    and no spilled register.  The compiler's account only, not the assembly."""
    if not os.path.isdir(os.path.dirname(RESOURCES)):
        pytest.skip("the build directory %s is absent" % os.path.dirname(RESOURCES))
    assert os.path.exists(RESOURCES), "%s is missing: the build writes it for every .hip source" % RESOURCES
    src = _read(os.path.join(ROOT, "kmer-db_amd", "csrc", "build.hip")).decode()
    kernels = set(re.findall(r"\bvoid (bd_\w+_kernel)\(", src))
    assert len(kernels) >= 15, sorted(kernels)
    found, cur = {}, None
    with open(RESOURCES, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.match(r"_ZN12_GLOBAL__N_1\d+(bd_\w+_kernel)E", m.group(1))
                cur = found.setdefault(k.group(1), {}) if k else None
                continue
            m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
    assert set(found) == kernels, (sorted(kernels - set(found)), sorted(set(found) - kernels))
    for key, r in sorted(found.items()):
        print(key, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (key, r)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
_SHAPE_CACHE = {}


def _shape(S, O, shape, td):
    """(names, lists, the file to compare with, how it was made) of a shape, made once: the one-thread reference build of the same lists
    where the reference is built, else synth.write_db of synth.build_patterns"""
    if shape not in _SHAPE_CACHE:
        import torch
        n, clade, L, k, f = shape
        names, lists = BC.shape_lists(shape)
        if os.path.exists(REF_DRIVER):
            O.write_kmers_bin(os.path.join(td, "k.bin"), k, f, list(zip(names, lists)))
            O.ref_build(os.path.join(td, "k.bin"), os.path.join(td, "want.db"), 1)
            how = "reference"
        else:
            ts = [torch.from_numpy(x.view(np.int64)) for x in lists]
            pat = S.build_patterns(lambda i: ts[i], n, "cpu")
            S.write_db(os.path.join(td, "want.db"), k, f, names, pat["sample_counts"], S.to_view_arrays(pat), kmers_count=int(pat["dictionary"].numel()),
                       tables=S.build_hashtables(pat["dictionary"], pat["kmer_pid"], k))
            how = "synth"
        O.REF_BRANCHES["test_build.py:_shape"] = how == "reference"
        _SHAPE_CACHE[shape] = (names, lists, _read(os.path.join(td, "want.db")), how)
    return _SHAPE_CACHE[shape]


@pytest.fixture(scope="module")
def shape_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("build_shapes"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BC.SHAPES, ids=["N%d-k%d-f%g" % (s[0], s[3], s[4]) for s in BC.SHAPES])
def test_build_equals_the_one_thread_reference_build(K, S, O, dev, shape, shape_dir, tmp_path):
    """kmdb_build_add_kmers + finish + store against ref_build(..., threads=1) of the same lists: header + samples equal, patterns equal
    under the section compare, every bucket's set of items equal with well-formed tables, and the reference's find walks OUR tables"""
    n, clade, L, k, f = shape
    if _require_ref():
        conftest.require_ref_or_skip(REF_DRIVER, "needs the reference build (oracle/_ref/ref_driver)")
    names, lists, want, how = _shape(S, O, shape, shape_dir)
    h, st = _build(K, k, f, names, lists)
    out = str(tmp_path / "ours.db")
    h.store(out)
    got = _read(out)
    print(how, st)
    _same_sections(got, want, tables="content")
    assert st["distinct_kmers"] == np.unique(np.concatenate(lists)).size and st["patterns"] == BC.split_db(want)["P"]
    # the view's arrays against the restatement in synth (always, whatever made `want`)
    import torch
    ts = [torch.from_numpy(x.view(np.int64)) for x in lists]
    arr = S.to_view_arrays(S.build_patterns(lambda i: ts[i], n, "cpu"))
    mine = h.view_arrays()
    for key in ("num_kmers", "parent_id", "num_samples", "num_local", "last_sample_id", "num_bits", "data_offset", "data"):
        assert np.array_equal(mine[key], arr[key]), key
    # queries: ten of the samples through OUR tables
    qs = [lists[i] for i in range(0, n, max(1, n // 10))][:10]
    want_path = str(tmp_path / "want.db")
    with open(want_path, "wb") as fh:
        fh.write(want)
    odb, wdb = O.OracleDB(out), O.OracleDB(want_path)
    for q in qs:
        assert np.array_equal(odb.one2all(q), wdb.one2all(q))
    if how == "reference":
        _queries_bin(O, str(tmp_path / "q.bin"), k, f, qs)
        ra, _ = O.ref_one2all(out, str(tmp_path / "q.bin"), str(tmp_path / "ra.u32"))
        rb, _ = O.ref_one2all(want_path, str(tmp_path / "q.bin"), str(tmp_path / "rb.u32"))
        assert ra.size == len(qs) * n and np.array_equal(ra, rb)


@pytest.mark.gpu
def test_batch_boundaries_do_not_matter(K, S, O, dev, shape_dir, tmp_path):
    """the first shape added in one call, in calls of 1, of 7 and of 1, 2, 4, 8, ...: four identical files (the dictionary merge sees new
    k-mers before, between and after everything it holds)"""
    shape = BC.SHAPES[0]
    n, clade, L, k, f = shape
    names, lists, want, how = _shape(S, O, shape, shape_dir)
    pow2, left = [], n
    while left:
        pow2.append(min(left, 1 << len(pow2)))
        left -= pow2[-1]
    files = []
    for tag, calls in (("one", None), ("ones", [1] * n), ("sevens", [7] * (n // 7) + ([n % 7] if n % 7 else [])), ("pow2", pow2)):
        h, st = _build(K, k, f, names, lists, calls)
        p = str(tmp_path / (tag + ".db"))
        h.store(p)
        files.append(_read(p))
    assert files[0] == files[1] == files[2] == files[3]
    _same_sections(files[0], want, tables="content")


def _headers_of(h):
    v = h.view_arrays()
    P = v["num_kmers"].size
    parents = {int(p) for p in v["parent_id"] if p >= 0}
    return [(int(v["num_kmers"][p]), int(v["parent_id"][p]), int(v["num_samples"][p]), int(v["num_local"][p]), int(v["last_sample_id"][p]),
             int(v["num_bits"][p]), 1 if p in parents else 0) for p in range(P)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BC.TREES, ids=[re.sub(r"\W+", "-", t[0])[:40] for t in BC.TREES])
def test_rules_of_the_tree(K, S, dev, case, tmp_path):
    """hand-made lists, the expected headers written out by hand (build_cases.TREES) and cross-checked with synth.build_patterns; the stored
    file carries the same headers, is_parent included, and the empty samples keep their id, name and count 0"""
    import torch
    what, lists, expected = case
    names = ["s%d" % i for i in range(len(lists))]
    arrs = [np.array(x, dtype=np.uint64) for x in lists]
    ts = [torch.from_numpy(x.view(np.int64)) for x in arrs]
    pat = S.build_patterns(lambda i: ts[i], len(ts), "cpu")
    arr = S.to_view_arrays(pat)
    for col, key in enumerate(("num_kmers", "parent_id", "num_samples", "num_local", "last_sample_id", "num_bits")):
        assert [int(x) for x in arr[key]] == [e[col] for e in expected], (what, key)
    for calls in (None, [1] * len(lists)):
        h, st = _build(K, 18, 1.0, names, arrs, calls)
        assert _headers_of(h) == expected, what
        assert h.names == names and [int(x) for x in h.sample_kmers] == [len(x) for x in lists]
        p = str(tmp_path / "t.db")
        h.store(p)
        assert [tuple(f) for f in BC.pattern_headers(BC.split_db(_read(p))["patterns_raw"])] == expected, what


def _local_ids(O, v, p):
    """the local ids of pattern p decoded from the view's stream: the first id is not coded, the last one is stored"""
    l, bits, last = int(v["num_local"][p]), int(v["num_bits"][p]), int(v["last_sample_id"][p])
    if l == 0:
        return []
    words = ((bits + 127) // 128) * 2 if bits else 0
    off = int(v["data_offset"][p])
    deltas = O.gamma_decode(v["data"][off: off + max(words, 2)], bits, max(l, 1)).astype(np.int64) if bits else np.zeros(0, np.int64)
    assert deltas.size == l - 1
    ids = last - (deltas.sum() - np.concatenate([[0], np.cumsum(deltas)]))
    return [int(x) for x in ids]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BC.gamma_cases(), ids=[re.sub(r"\W+", "-", c[0])[:40] for c in BC.gamma_cases()])
def test_gamma_streams_at_their_edges(K, O, dev, case, tmp_path):
    """every stream decoded back with the oracle's decoder; with the reference build present, the file against ref_build(..., 1)"""
    what, n, samples, expected = case
    names = ["s%d" % i for i in range(n)]
    empty = np.zeros(0, np.uint64)
    lists = [np.array(samples[s], dtype=np.uint64) if s in samples else empty for s in range(n)]
    h, st = _build(K, 18, 1.0, names, lists)
    v = h.view_arrays()
    assert v["num_kmers"].size == len(expected) + 1, what
    for p, ids in expected.items():
        bits = BC.stream_bits(ids)
        assert int(v["num_bits"][p]) == bits and int(v["num_local"][p]) == len(ids) and int(v["last_sample_id"][p]) == ids[-1], (what, p)
        assert _local_ids(O, v, p) == ids, (what, p)
    assert int(v["data"].size) == 2 + sum(((BC.stream_bits(ids) + 127) // 128) * 2 for ids in expected.values())     # each stream padded on its own
    out = str(tmp_path / "g.db")
    h.store(out)
    odb = O.OracleDB(out)
    for p, ids in expected.items():
        if int(v["parent_id"][p]) < 0:
            assert [int(x) for x in odb.decode_chain(p)] == ids, (what, p)
    if os.path.exists(REF_DRIVER):
        O.write_kmers_bin(str(tmp_path / "k.bin"), 18, 1.0, list(zip(names, lists)))
        O.ref_build(str(tmp_path / "k.bin"), str(tmp_path / "r.db"), 1)
        _same_sections(_read(out), _read(str(tmp_path / "r.db")), tables="content")
    elif _require_ref():
        pytest.fail("KMDB_REQUIRE_REF=1: %s is missing" % REF_DRIVER)


def _finds_everything(O, path, lists, kmer_pid=None):
    """OracleDB.one2all of every sample on the file == the counts from the lists themselves: every k-mer is found, with the right pattern"""
    odb = O.OracleDB(path)
    sets = [set(int(x) for x in q) for q in lists]
    for q in lists:
        want = [len(set(int(x) for x in q) & s) for s in sets]
        assert [int(x) for x in odb.one2all(np.asarray(q, np.uint64))] == want
    odb.close()


def _ref_finds_everything(O, path, k, f, lists, tmp_path):
    if not os.path.exists(REF_DRIVER):
        if _require_ref():
            pytest.fail("KMDB_REQUIRE_REF=1: %s is missing" % REF_DRIVER)
        return
    sets = [set(int(x) for x in q) for q in lists]
    _queries_bin(O, str(tmp_path / "q.bin"), k, f, [np.asarray(q, np.uint64) for q in lists])
    r, _ = O.ref_one2all(path, str(tmp_path / "q.bin"), str(tmp_path / "r.u32"))
    want = [len(set(int(x) for x in q) & s) for q in lists for s in sets]
    assert [int(x) for x in r] == want


@pytest.mark.gpu
@pytest.mark.parametrize("case", BC.table_cases(), ids=[re.sub(r"\W+", "-", c[0])[:40] for c in BC.table_cases()])
def test_tables_at_their_edges(K, O, dev, case, tmp_path):
    what, k, lists, caps = case
    arrs = [np.array(x, dtype=np.uint64) for x in lists]
    h, st = _build(K, k, 1.0, ["s%d" % i for i in range(len(arrs))], arrs)
    out = str(tmp_path / "t.db")
    h.store(out)
    x = BC.split_db(_read(out))
    BC.assert_tables_well_formed(x["tables"])
    assert x["n_buckets"] == 1 << max(8, 2 * k - 32)
    distinct = np.unique(np.concatenate(arrs))
    for b, (hdr, bv, items) in enumerate(x["tables"]):
        assert hdr[2] == caps.get(b, 16), (what, b, hdr)
        assert hdr[1] == int(((distinct >> np.uint64(32)) == np.uint64(b)).sum())
    _finds_everything(O, out, arrs)
    _ref_finds_everything(O, out, k, 1.0, arrs, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("k,f,n_buckets", [(12, 1.0, 256), (25, 0.1, 1 << 18)])
def test_tables_of_short_and_long_kmers(K, S, O, dev, tmp_path, k, f, n_buckets):
    """k = 12: 24-bit k-mers widened to 40 bits, 256 buckets; a second builder holds only k-mers of bucket 0, every other table stays the
    empty table's header.  k = 25, f = 0.1: 2^18 buckets, most of them empty."""
    g = S.CladeGenomes(6, 3, 3000, seed=11)
    lists = [S.kmers_of(g.sample(i), k, f).numpy().view(np.uint64).copy() for i in range(6)]
    h, st = _build(K, k, f, [g.name(i) for i in range(6)], lists)
    out = str(tmp_path / "t.db")
    h.store(out)
    x = BC.split_db(_read(out))
    assert x["n_buckets"] == n_buckets
    BC.assert_tables_well_formed(x["tables"])
    assert sum(t[0][1] for t in x["tables"]) == st["distinct_kmers"]
    if k == 25:
        assert sum(1 for t in x["tables"] if t[0][1] == 0) > n_buckets // 2
    _finds_everything(O, out, lists)
    _ref_finds_everything(O, out, k, f, lists, tmp_path)
    if k == 12:
        low = [np.array(sorted(q), dtype=np.uint64) for q in ([5, 9, 77, 1 << 20, (1 << 32) - 1], [9, 10, 11], [(1 << 32) - 1])]
        h, st = _build(K, 12, 1.0, ["a", "b", "c"], low)
        h.store(out)
        x = BC.split_db(_read(out))
        assert x["tables"][0][0][1] == 7 and all(t[0][1:3] == (0, 16) and not t[2].size for t in x["tables"][1:])
        _finds_everything(O, out, low)
        _ref_finds_everything(O, out, 12, 1.0, low, tmp_path)


def _fasta_records(text):
    recs = []
    for block in text.split(">")[1:]:
        head, _, body = block.partition("\n")
        recs.append((head.split(" ")[0].strip(), body.replace("\n", "").replace("\r", "")))
    return recs


TEXT_CASES = [("synth.synth.fa", "synth_k21")] + [("protein.aa_100x1000.fasta.xz", "protein_" + a) for a in ("aa", "aa11_diamond", "aa12_mmseqs", "aa6_dayhoff", "aa_k7")]


@pytest.mark.gpu
@pytest.mark.parametrize("fasta,stem", TEXT_CASES, ids=[c[1] for c in TEXT_CASES])
def test_text_in_equals_lists_in(K, dev, golden_dir, tmp_path, fasta, stem):
    """kmdb_build_add_seq_alphabet on the records of a FASTA file == kmdb_build_add_kmers on kmdbh_extract_kmers_alphabet +
    kmdbh_sort_unique of the same text, file for file; k, fraction and alphabet from the matching golden database"""
    src = os.path.join(ROOT, "tests", "golden", fasta)
    text = (lzma.open(src).read() if fasta.endswith(".xz") else _read(src)).decode()
    recs = _fasta_records(text)
    g = K.HostDB(os.path.join(golden_dir, stem + ".db"), skip_hashtables=True)
    k, f, alphabet = g.k, g.fraction, K.ALPHABETS[g.alphabet]
    names = [r[0] for r in recs]
    assert names == g.names
    lists = [K.sort_unique(K.extract_kmers_alphabet(r[1].encode(), k, alphabet, f)) for r in recs]
    assert [len(x) for x in lists] == [int(x) for x in g.sample_kmers]
    h1, _ = _build(K, k, f, names, lists, alphabet=alphabet)
    b = K.Builder(k, f, 0.0, alphabet)
    half = len(recs) // 2
    b.add_seqs(names[:half], [r[1] + "\n" for r in recs[:half]])
    b.add_seqs(names[half:], [r[1] + "\n" for r in recs[half:]])
    h2 = b.finish()
    b.close()
    h1.store(str(tmp_path / "lists.db"))
    h2.store(str(tmp_path / "text.db"))
    assert _read(str(tmp_path / "lists.db")) == _read(str(tmp_path / "text.db"))
    # and the golden database (built by the reference from the same records) holds the same patterns up to their order
    a, c = h2.view_arrays(), g.view_arrays()
    key = lambda v: sorted(zip(v["num_kmers"].tolist(), v["num_samples"].tolist(), v["num_local"].tolist(), v["last_sample_id"].tolist(), v["num_bits"].tolist()))  # noqa: E731
    assert key(a) == key(c)


@pytest.mark.gpu
def test_build_upload_compare_without_a_disk(K, S, O, dev, shape_dir, tmp_path):
    """finish -> kmdb_db_upload(kmdbh_db_view(h), ..., 1): all2all and new2all on the resident database equal the oracle on the reference-built file"""
    shape = BC.SHAPES[0]
    n, clade, L, k, f = shape
    names, lists, want, how = _shape(S, O, shape, shape_dir)
    h, st = _build(K, k, f, names, lists)
    d = K.DeviceDB(h, device=dev, with_hashtables=True)
    with open(str(tmp_path / "want.db"), "wb") as fh:
        fh.write(want)
    odb = O.OracleDB(str(tmp_path / "want.db"))
    assert np.array_equal(d.all2all_dense(), odb.all2all_dense())
    qs = [lists[i] for i in (0, 5, 17, 30, n - 1)]
    assert np.array_equal(d.new2all(qs), np.stack([odb.one2all(q) for q in qs]))
    d.close()


@pytest.mark.gpu
def test_front_end_workflows(K, dev, golden_dir, tmp_path):
    """the reference's own test workflows (test/run-dev.bat, run-synth.bat) through `kmer-db-amd build`"""
    root = MC.link_virus_data(golden_dir, str(tmp_path))
    g = lambda n: os.path.join(golden_dir, n)          # noqa: E731
    t = lambda n: str(tmp_path / n)                    # noqa: E731
    r = _cli("build", "-k", "18", g("virus.seqs.list"), t("v.db"), cwd=root)
    for line in ("Building database (from fasta genomes)", "Processing samples...", "EXECUTION TIMES", "Serializing database..."):
        assert line in r.stderr
    _cli("all2all", t("v.db"), t("v.csv"))
    assert _read(t("v.csv")) == _read(g("virus.k18.csv"))
    _cli("build", "-f", "0.1", g("virus.seqs.list"), t("vf.db"), cwd=root)
    _cli("all2all", t("vf.db"), t("vf.csv"))
    assert _read(t("vf.csv")) == _read(g("virus.k18.frac.csv"))
    # the host extractor gives the same file as the device extractor, and the golden database's patterns
    _cli("build", "-host-extract", "-f", "0.1", "-t", "4", g("virus.seqs.list"), t("vfh.db"), cwd=root)
    assert _read(t("vfh.db")) == _read(t("vf.db"))
    # -multisample-fasta: every record a sample, named by its header
    with open(t("synth.list"), "w") as f:
        f.write(g("synth.synth") + "\n")
    _cli("build", "-multisample-fasta", "-k", "21", t("synth.list"), t("s.db"))
    _cli("all2all", t("s.db"), t("s.a2a"))
    assert _read(t("s.a2a")) == _read(g("synth.a2a"))
    # minhash, then build -from-minhash == build -f with the same fraction, k and alphabet
    _cli("minhash", "-k", "18", "-f", "0.1", g("virus.seqs.list"), cwd=root)
    r = _cli("build", "-from-minhash", g("virus.seqs.list"), t("vm.db"), cwd=root)
    assert "Building database (from minhashed k-mers)" in r.stderr
    assert _read(t("vm.db")) == _read(t("vf.db"))
    # -f-start: the start the builder used is in the header (the reference writes 0 there)
    entries = MC.virus_entries(golden_dir)
    with open(t("few.list"), "w") as f:
        f.write("\n".join(entries[:3]) + "\n")
    _cli("build", "-f", "0.2", "-f-start", "0.3", t("few.list"), t("fs.db"), cwd=root)
    h = K.HostDB(t("fs.db"))
    assert (h.fraction, h.start_fraction, h.N) == (0.2, 0.3, 3)
    # a list with one unreadable entry: reported, and the others are numbered consecutively
    with open(t("gap.list"), "w") as f:
        f.write("%s\n./test/virus/data/NO_SUCH_GENOME\n%s\n" % (entries[0], entries[1]))
    r = _cli("build", t("gap.list"), t("gap.db"), cwd=root)
    assert "failed:./test/virus/data/NO_SUCH_GENOME" in r.stderr
    with open(t("two.list"), "w") as f:
        f.write("%s\n%s\n" % (entries[0], entries[1]))
    _cli("build", t("two.list"), t("two.db"), cwd=root)
    assert _read(t("gap.db")) == _read(t("two.db"))
    assert K.HostDB(t("gap.db")).names == [os.path.basename(e) for e in entries[:2]]
    # files of another k or fraction end the run with the reference's message
    _cli("minhash", "-k", "20", "-f", "0.2", t("few.list"), cwd=root)
    _cli("minhash", "-k", "20", "-f", "0.1", t("two.list"), cwd=root)          # the first two at 0.1, the third of few.list stays at 0.2
    r = _cli("build", "-from-minhash", t("few.list"), t("bad.db"), cwd=root, ok=False)
    assert r.returncode != 0 and "adding kmers of different minhash fraction" in r.stderr


@pytest.mark.gpu
def test_refusals_on_the_device_path(K, dev, monkeypatch):
    """status checks on valid memory: an unsorted list, a duplicate, an add after finish, a state that does not fit — each an error with
    kmdb_last_error set; the first three leave the builder as it was, the last leaves it dead"""
    a = np.array([5, 9, 12, 40], np.uint64)
    b = K.Builder(18)
    b.add_kmers(["s0"], [a])
    with pytest.raises(K.KmdbError, match="sample bad are not strictly ascending"):
        b.add_kmers(["ok", "bad"], [a, np.array([5, 12, 9], np.uint64)])
    with pytest.raises(K.KmdbError, match="sample dup are not strictly ascending"):
        b.add_kmers(["dup"], [np.array([5, 9, 9, 12], np.uint64)])
    assert b.stats()["samples"] == 1                                   # nothing of the refused calls was added
    b.add_kmers(["s1", "s2"], [a, np.zeros(0, np.uint64)])             # a list that ends where the next begins lower is fine
    b.add_kmers(["s3", "s4"], [np.array([50, 60], np.uint64), np.array([1, 2], np.uint64)])
    h = b.finish()
    assert h.names == ["s0", "s1", "s2", "s3", "s4"] and [int(x) for x in h.sample_kmers] == [4, 4, 0, 2, 2]
    with pytest.raises(K.KmdbError, match="finished"):
        b.add_kmers(["late"], [a])
    with pytest.raises(K.KmdbError, match="finished"):
        b.finish()
    b.close()
    for k, alphabet, word in ((32, "nt", "k-mer length must be 1..31"), (12, "aa", "k-mer length must be 1..11"), (18, 17, "unknown alphabet")):
        with pytest.raises(K.KmdbError, match=word):
            K.Builder(k, 1.0, 0.0, alphabet)
    # a collection whose state does not fit: the error names the bytes, the builder is dead afterwards
    monkeypatch.setenv("KMDB_BUILD_DEVICE_BYTES", str(4 << 20))
    b = K.Builder(18)
    monkeypatch.delenv("KMDB_BUILD_DEVICE_BYTES")
    b.add_kmers(["small"], [a])
    big = np.arange(1, 400001, dtype=np.uint64) * np.uint64(3)
    with pytest.raises(K.KmdbError, match=r"does not fit the device: \d+ bytes needed for"):
        b.add_kmers(["big"], [big])
    with pytest.raises(K.KmdbError, match="dead"):
        b.add_kmers(["again"], [a])
    with pytest.raises(K.KmdbError, match="dead"):
        b.finish()
    b.close()
