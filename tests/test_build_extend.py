"""build -extend-from: kmdb_build_begin_from_db (csrc/build.hip) seeds a builder from a stored database, on the device.

Correctness is defined by the rebuild: extending build(A) with the samples B gives the file that build(A followed by B) gives, byte for
byte, tables included (both come from this builder with one pattern task: the ids are the one-thread ids).  The reference's own `-extend`
is no byte-level witness (pattern_t::unpack leaves is_parent to the stack, pattern.cpp:77-79); its workflow is checked through all2all /
new2all on the extended database, as its CI does.  Helpers live in tests/extend_cases.py, inputs in tests/build_cases.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import build_cases as BC
import conftest
import extend_cases as EC
import minhash_cases as MC
from conftest import ROOT

EXE = os.path.join(ROOT, "kmer-db_amd", "bin", "kmer-db-amd")
RESOURCES = os.path.join(ROOT, "kmer-db_amd", "build", "build.resources.txt")
REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
HEADER = os.path.join(ROOT, "include", "kmdb_amd.h")
SEED_KERNELS = ("bd_seed_flag_kernel", "bd_seed_compact_kernel", "bd_seed_isp_kernel", "bd_seed_dict_check_kernel", "bd_seed_count_check_kernel",
                "bd_seed_decode_kernel")
EMPTY = np.zeros(0, np.uint64)


@pytest.fixture(scope="module")
def dev(K):
    assert K.device_count() > 0, "the -m gpu tests need an MI355X; the engine has no CPU fallback"
    return 0


def _cli(*args, cwd=None, ok=True, env=None):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, cwd=cwd, env=env)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_declared(K):
    import ctypes
    src = EC.read(HEADER).decode()
    assert re.search(r"^#define KMDB_HAS_BUILD_SEED 1$", src, re.M)
    assert re.search(r"^#define KMDB_ABI_VERSION 8$", src, re.M)
    assert K.ABI_VERSION == 8 and K.lib().kmdb_abi_version() == 8
    L = ctypes.CDLL(K.lib_path())
    for name in ("kmdb_build_begin_from_db", "kmdb_build_seed_stats_get"):
        assert name in K.capi.EXPORTS and hasattr(L, name)
        assert re.search(r"^int\s+%s\(" % name, src, re.M), name
    assert all(hasattr(L, name) for name in K.capi.EXPORTS)
    # the struct of the binding is the struct of the header: six u64, then five f64
    m = re.search(r"typedef struct kmdb_build_seed_stats \{(.*?)\} kmdb_build_seed_stats;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decl = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|double)\s+([^;]+);", body) for n in names.split(",")]
    assert decl == [({"c_ulong": "uint64_t", "c_double": "double"}[t.__name__], f) for f, t in K.capi._BuildSeedStats._fields_]
    assert hasattr(K.Builder, "from_db") and hasattr(K.Builder, "seed_stats")


def test_cli_refuses_a_missing_database_before_any_device(tmp_path):
    lst, db = str(tmp_path / "x.list"), str(tmp_path / "x.db")
    with open(lst, "w") as f:
        f.write("nothing\n")
    r = _cli("build", "-extend-from", str(tmp_path / "no_such.db"), lst, db, ok=False)
    assert r.returncode not in (0, -11, -6) and "ERROR: Cannot open k-mer database " + str(tmp_path / "no_such.db") in r.stderr, r.stderr
    assert not os.path.exists(db)
    r = _cli("build", "-extend-from", str(tmp_path / "no_such.db"), lst, ok=False)             # a missing argument
    assert r.returncode != 0 and "USAGE" in r.stderr
    r = _cli()
    assert "build -extend-from <old.db>" in r.stderr and "-extend and -from-kmers are refused" in r.stderr


def test_a_database_without_tables_is_refused_on_the_host(K, golden_dir):
    """before any device work: this runs where there is no device"""
    h = K.HostDB(os.path.join(golden_dir, "virus_k18_part1.db"), skip_hashtables=True)
    with pytest.raises(K.KmdbError, match="kmdb_build_begin_from_db: the database holds no hashtables"):
        K.Builder.from_db(h)


def test_seed_kernels_use_no_scratch():
    """the compiler's resource remarks list every kernel of the seed with a scratch size of 0 and no spilled register"""
    if not os.path.isdir(os.path.dirname(RESOURCES)):
        pytest.skip("the build directory %s is absent" % os.path.dirname(RESOURCES))
    assert os.path.exists(RESOURCES), "%s is missing: the build writes it for every .hip source" % RESOURCES
    src = EC.read(os.path.join(ROOT, "kmer-db_amd", "csrc", "build.hip")).decode()
    assert set(re.findall(r"\bvoid (bd_seed_\w+_kernel)\(", src)) == set(SEED_KERNELS)
    found, cur = {}, None
    with open(RESOURCES, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.match(r"_ZN12_GLOBAL__N_1\d+(bd_seed_\w+_kernel)E", m.group(1))
                cur = found.setdefault(k.group(1), {}) if k else None
                continue
            m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
    assert set(found) == set(SEED_KERNELS), sorted(set(SEED_KERNELS) - set(found))
    for key, r in sorted(found.items()):
        print(key, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (key, r)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
_SHAPES = {}


def _shape(K, shape, td):
    """(names, lists, the file of the one-call build of the whole list), made once per shape"""
    if shape not in _SHAPES:
        names, lists = BC.shape_lists(shape)
        full, st = EC.build_file(K, shape[3], shape[4], names, lists, os.path.join(td, "full%d.db" % len(_SHAPES)))
        _SHAPES[shape] = (names, lists, full, st)
    return _SHAPES[shape]


@pytest.fixture(scope="module")
def shape_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("extend_shapes"))


@pytest.mark.gpu
def test_seed_then_finish_changes_nothing(K, dev, shape_dir, tmp_path, monkeypatch):
    """store(from_db(load(f)).finish()) == f for a file built here, whatever the size of the pieces the slots go up in"""
    shape = BC.SHAPES[0]
    names, lists, full, st = _shape(K, shape, shape_dir)
    src, out = str(tmp_path / "f.db"), str(tmp_path / "g.db")
    with open(src, "wb") as f:
        f.write(full)
    n_slots = sum(t[0][2] for t in BC.split_db(full)["tables"])
    for piece in (None, 1000, 4096, n_slots - 1, n_slots):
        if piece is None:
            monkeypatch.delenv("KMDB_BUILD_SEED_SLOTS_PER_PIECE", raising=False)
        else:
            monkeypatch.setenv("KMDB_BUILD_SEED_SLOTS_PER_PIECE", str(piece))
        got, st2 = EC.extend_file(K, src, [], [], out)
        assert got == full, piece
        for key in ("samples", "distinct_kmers", "patterns", "events"):
            assert st2[key] == st[key], key
        assert st2["kmers_added"] == 0
    monkeypatch.delenv("KMDB_BUILD_SEED_SLOTS_PER_PIECE", raising=False)
    h = K.HostDB(src)
    b = K.Builder.from_db(h)
    seed = b.seed_stats()
    print(seed)
    assert seed["slots"] == n_slots and seed["distinct_kmers"] == st["distinct_kmers"] and seed["events"] == st["events"]
    assert seed["h2d_bytes"] >= 8 * n_slots + 12 * st["patterns"]
    b.close()
    assert K.Builder(18).seed_stats()["samples"] == 0              # zeros on a builder that was not seeded


@pytest.mark.gpu
def test_seed_from_a_database_in_the_reference_layout(K, dev, golden_dir, tmp_path):
    """virus_k18_part1.db was built by the reference with four threads: other capacities, pattern ids in no one-thread order.  Seed and
    finish: header and samples equal, patterns equal under the section compare, every bucket's items equal in well-formed tables"""
    src, out = os.path.join(golden_dir, "virus_k18_part1.db"), str(tmp_path / "g.db")
    got, st = EC.extend_file(K, src, [], [], out)
    EC.same_sections(got, EC.read(src), tables="content")
    assert st["samples"] == 100 and st["patterns"] == BC.split_db(got)["P"]


CUTS = [(si, cut) for si in range(len(BC.SHAPES)) for cut in ("1", "mid", "N-1")]


@pytest.mark.gpu
@pytest.mark.parametrize("si,cut", CUTS, ids=["N%d-k%d-cut-%s" % (BC.SHAPES[si][0], BC.SHAPES[si][3], cut) for si, cut in CUTS])
def test_extension_equals_rebuild(K, dev, shape_dir, tmp_path, si, cut):
    shape = BC.SHAPES[si]
    n, clade, L, k, f = shape
    names, lists, full, st = _shape(K, shape, shape_dir)
    c = {"1": 1, "mid": n // 2, "N-1": n - 1}[cut]
    head, out = str(tmp_path / "head.db"), str(tmp_path / "ext.db")
    EC.build_file(K, k, f, names[:c], lists[:c], head)
    tail = n - c
    for calls in [None] + ([[tail // 2, tail - tail // 2]] if tail > 1 else []):
        got, st2 = EC.extend_file(K, head, names[c:], lists[c:], out, calls)
        assert got == full, (cut, calls)
        for key in ("samples", "distinct_kmers", "patterns", "events"):
            assert st2[key] == st[key], key
        assert st2["kmers_added"] == sum(len(x) for x in lists[c:])


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(BC.SHAPES)), ids=["N%d-k%d" % (s[0], s[3]) for s in BC.SHAPES])
def test_extension_equals_the_one_thread_reference_build(K, O, dev, shape_dir, tmp_path, si):
    """the extended file against ref_build(..., threads=1) of the whole list under the section compare: patterns masked, tables by content"""
    conftest.require_ref_or_skip(REF_DRIVER, "needs the reference build (oracle/_ref/ref_driver)")
    shape = BC.SHAPES[si]
    n, clade, L, k, f = shape
    names, lists, full, st = _shape(K, shape, shape_dir)
    O.write_kmers_bin(str(tmp_path / "k.bin"), k, f, list(zip(names, lists)))
    O.ref_build(str(tmp_path / "k.bin"), str(tmp_path / "ref.db"), 1)
    head, out = str(tmp_path / "head.db"), str(tmp_path / "ext.db")
    EC.build_file(K, k, f, names[:n // 2], lists[:n // 2], head)
    got, _ = EC.extend_file(K, head, names[n // 2:], lists[n // 2:], out)
    assert got == full
    EC.same_sections(got, EC.read(str(tmp_path / "ref.db")), tables="content")


@pytest.mark.gpu
def test_extending_twice(K, dev, shape_dir, tmp_path):
    """A, + B, + C: every stored file is loaded again before it is extended"""
    shape = BC.SHAPES[0]
    n, clade, L, k, f = shape
    names, lists, full, st = _shape(K, shape, shape_dir)
    a, b = n // 3, 2 * n // 3
    p0, p1, p2 = (str(tmp_path / x) for x in ("a.db", "ab.db", "abc.db"))
    EC.build_file(K, k, f, names[:a], lists[:a], p0)
    EC.extend_file(K, p0, names[a:b], lists[a:b], p1)
    got, _ = EC.extend_file(K, p1, names[b:], lists[b:], p2)
    assert got == full
    # and in place: the file that is read is the file that is written
    EC.extend_file(K, p0, names[a:b], lists[a:b], p0)
    assert EC.read(p0) == EC.read(p1)


# the seed of every tree case: s0 = {1, 2, 3, 4} -> pattern 1; s1 = {1, 2, 5}: {5} -> pattern 2 (parent -1), {1, 2} -> pattern 3, child of 1,
# which keeps {3, 4} and becomes a parent.  P = 4, three events.  (what, the added sample, patterns afterwards, events afterwards)
SEAM = [
    ("a childless pattern taken whole is extended in place", [5], 4, 4),
    ("a parent taken whole: a new pattern (an extension if is_parent were seeded as zeros)", [3, 4], 5, 4),
    ("a split", [3], 5, 4),
    ("only new k-mers: the parent is -1", [7, 8], 5, 4),
    ("an empty sample takes an id and no event", [], 4, 3),
    # groups by old id: 0 {7} -> 4; 1 {3, 4}, whole but a parent -> 5; 2 {5} extended; 3 {1, 2} extended
    ("several groups in one sample", [1, 2, 3, 4, 5, 7], 6, 7),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEAM, ids=[re.sub(r"\W+", "-", c[0])[:40] for c in SEAM])
def test_rules_of_the_tree_across_the_seam(K, dev, case, tmp_path):
    what, added, P, E = case
    seed_lists = [np.array(x, np.uint64) for x in ([1, 2, 3, 4], [1, 2, 5])]
    new = np.array(added, np.uint64)
    head, out, full = (str(tmp_path / x) for x in ("head.db", "ext.db", "full.db"))
    _, st0 = EC.build_file(K, 18, 1.0, ["s0", "s1"], seed_lists, head)
    assert (st0["patterns"], st0["events"]) == (4, 3)
    want, st = EC.build_file(K, 18, 1.0, ["s0", "s1", "s2"], seed_lists + [new], full)
    h, st2, seed = EC.extend(K, head, ["s2"], [new])
    h.store(out)
    assert EC.read(out) == want, what
    assert (st2["patterns"], st2["events"], st2["samples"]) == (P, E, 3) == (st["patterns"], st["events"], st["samples"]), what
    v = h.view_arrays()
    if added == [7, 8]:
        assert int(v["parent_id"][4]) == -1 and int(v["num_kmers"][4]) == 2
    if added == [3, 4]:
        assert int(v["parent_id"][4]) == 1 and int(v["num_kmers"][1]) == 0 and int(v["num_kmers"][4]) == 2
    if added == [1, 2, 3, 4, 5, 7]:
        assert [int(x) for x in v["parent_id"]] == [-1, -1, -1, 1, -1, 1] and [int(x) for x in v["num_samples"]] == [0, 1, 2, 3, 1, 2]
    assert h.names == ["s0", "s1", "s2"] and [int(x) for x in h.sample_kmers] == [4, 3, len(added)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BC.gamma_cases(), ids=[re.sub(r"\W+", "-", c[0])[:40] for c in BC.gamma_cases()])
def test_gamma_streams_across_the_seam(K, O, dev, case, tmp_path):
    """all samples but the last are stored, reloaded and decoded by the seed; the last one is added: lists of one id, codes over 32 bits,
    codes that straddle a word and padded streams all pass through bd_seed_decode_kernel and come back out of bd_write_codes_kernel"""
    what, n, samples, expected = case
    names = ["s%d" % i for i in range(n)]
    lists = [np.array(samples[s], dtype=np.uint64) if s in samples else EMPTY for s in range(n)]
    assert len(lists[-1]), "the case's last sample carries k-mers"
    head, out, full = (str(tmp_path / x) for x in ("head.db", "ext.db", "full.db"))
    want, st = EC.build_file(K, 18, 1.0, names, lists, full)
    EC.build_file(K, 18, 1.0, names[:-1], lists[:-1], head)
    h, st2, seed = EC.extend(K, head, names[-1:], lists[-1:])
    h.store(out)
    assert EC.read(out) == want, what
    assert seed["events"] == st["events"] - sum(1 for ids in expected.values() if ids[-1] == n - 1)
    v = h.view_arrays()
    assert v["num_kmers"].size == len(expected) + 1
    for p, ids in expected.items():
        assert EC.local_ids(O, v, p) == ids, (what, p)
    # and a seed of the whole database decodes every stream to its end
    h3, st3, seed3 = EC.extend(K, full, [], [])
    v3 = h3.view_arrays()
    for p, ids in expected.items():
        assert EC.local_ids(O, v3, p) == ids, (what, p)
    assert seed3["events"] == st["events"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BC.table_cases(), ids=[re.sub(r"\W+", "-", c[0])[:40] for c in BC.table_cases()])
def test_tables_across_the_seam(K, O, dev, case, tmp_path):
    """the seed is the database without the case's last sample (an empty sample goes first, so that the seed of a one-sample case is a
    database with a sample in it); the last sample is added to it: the bucket's capacity is decided during the extension"""
    what, k, lists, caps = case
    arrs = [EMPTY] + [np.array(x, dtype=np.uint64) for x in lists]
    names = ["s%d" % i for i in range(len(arrs))]
    head, out, full = (str(tmp_path / x) for x in ("head.db", "ext.db", "full.db"))
    want, _ = EC.build_file(K, k, 1.0, names, arrs, full)
    EC.build_file(K, k, 1.0, names[:-1], arrs[:-1], head)
    got, _ = EC.extend_file(K, head, names[-1:], arrs[-1:], out)
    assert got == want, what
    x = BC.split_db(got)
    BC.assert_tables_well_formed(x["tables"])
    for b, (hdr, bv, items) in enumerate(x["tables"]):
        assert hdr[2] == caps.get(b, 16), (what, b, hdr)
    EC.finds_everything(O, out, arrs)


def _data_rows(raw):
    return [ln.split(",") for ln in raw.decode().splitlines()[2:] if ln]


@pytest.mark.gpu
def test_the_reference_workflow(K, dev, golden_dir, tmp_path):
    """the reference's CI (.github/workflows/main.yml:85-97, 130-135): build part 1, extend with part 2, all2all == k18.csv — with the seed
    read from the reference's own part-1 database"""
    root = MC.link_virus_data(golden_dir, str(tmp_path))
    g = lambda n: os.path.join(golden_dir, n)          # noqa: E731
    t = lambda n: str(tmp_path / n)                    # noqa: E731

    def check(db):
        _cli("all2all", db, t("a.csv"))
        assert EC.read(t("a.csv")) == EC.read(g("virus.k18.csv"))
        _cli("all2all", "-sparse", db, t("a.sp.csv"))
        assert EC.read(t("a.sp.csv")) == EC.read(g("virus.k18.sparse.csv"))

    env = dict(os.environ, KMDB_VERBOSE="1")
    r = _cli("build", "-extend-from", g("virus_k18_part1.db"), "-k", "25", g("virus.seqs.part2.list"), t("out.db"), cwd=root, env=env)
    for line in ("Building database (from fasta genomes)", "Loading k-mer database", "Processing samples...", "[kmdb] build: seeded from 100 samples", "Serializing database..."):
        assert line in r.stderr, r.stderr
    check(t("out.db"))
    h = K.HostDB(t("out.db"))
    part1, part2 = MC.virus_entries(golden_dir, "virus.seqs.part1.list"), MC.virus_entries(golden_dir, "virus.seqs.part2.list")
    assert h.k == 18 and h.N == len(part1) + len(part2) and len(part1) == 100
    assert h.names == [os.path.basename(e) for e in part1 + part2]
    h.close()
    # in place
    shutil.copyfile(g("virus_k18_part1.db"), t("inplace.db"))
    _cli("build", "-extend-from", t("inplace.db"), g("virus.seqs.part2.list"), t("inplace.db"), cwd=root)
    assert EC.read(t("inplace.db")) == EC.read(t("out.db"))
    # the host extractor
    _cli("build", "-extend-from", g("virus_k18_part1.db"), "-host-extract", "-t", "4", g("virus.seqs.part2.list"), t("host.db"), cwd=root)
    assert EC.read(t("host.db")) == EC.read(t("out.db"))
    # minhash files of the database's k and fraction (the mode's own default fraction is 0.01: the database's is 1)
    _cli("minhash", "-k", "18", "-f", "1", g("virus.seqs.part2.list"), cwd=root)
    r = _cli("build", "-extend-from", g("virus_k18_part1.db"), "-from-minhash", g("virus.seqs.part2.list"), t("mh.db"), cwd=root)
    assert "Building database (from minhashed k-mers)" in r.stderr
    assert EC.read(t("mh.db")) == EC.read(t("out.db"))
    # files of another k end the run with the message run_build prints for them
    _cli("minhash", "-k", "20", "-f", "1", g("virus.seqs.part2.list"), cwd=root)
    r = _cli("build", "-extend-from", g("virus_k18_part1.db"), "-from-minhash", g("virus.seqs.part2.list"), t("bad.db"), cwd=root, ok=False)
    assert r.returncode != 0 and "adding kmers of different length" in r.stderr and not os.path.exists(t("bad.db"))
    # new2all of part 2 against the extended database: its first 100 columns are the rows against part 1
    _cli("new2all", t("out.db"), g("virus.seqs.part2.list"), t("n2a.csv"), cwd=root)
    got, want = _data_rows(EC.read(t("n2a.csv"))), _data_rows(EC.read(g("virus.k18.n2a.csv")))
    assert len(got) == len(want) == len(part2)
    assert [r[:102] for r in got] == [r[:102] for r in want]
    # -extend keeps its refusal
    r = _cli("build", "-extend", g("virus.seqs.part2.list"), t("no.db"), cwd=root, ok=False)
    assert "build -extend is not supported: rebuild from the sample list" in r.stderr and not os.path.exists(t("no.db"))


@pytest.mark.gpu
def test_refusals_of_the_seed(K, dev, shape_dir, tmp_path, monkeypatch):
    """status checks on clamped reads: each a KmdbError with its message, no builder handed out; a good file seeds in the same process afterwards"""
    shape = BC.SHAPES[0]
    names, lists, full, st = _shape(K, shape, shape_dir)
    good, bad = str(tmp_path / "good.db"), str(tmp_path / "bad.db")
    with open(good, "wb") as f:
        f.write(full)
    P = BC.split_db(full)["P"]

    def refused(raw, word):
        with open(bad, "wb") as f:
            f.write(raw)
        try:
            h = K.HostDB(bad)
        except K.KmdbError as e:                                       # the loader's own refusal of the damaged file
            assert "Cannot open k-mer database" in str(e)
            return "loader"
        with pytest.raises(K.KmdbError, match=word):
            K.Builder.from_db(h)
        assert re.search(word, K.lib().kmdb_last_error().decode())
        h.close()
        return "seed"

    with pytest.raises(K.KmdbError, match="holds no hashtables"):
        K.Builder.from_db(K.HostDB(good, skip_hashtables=True))
    monkeypatch.setenv("KMDB_BUILD_DEVICE_BYTES", str(1 << 18))
    with pytest.raises(K.KmdbError, match=r"does not fit the device: \d+ bytes needed for"):
        K.Builder.from_db(K.HostDB(good))
    monkeypatch.delenv("KMDB_BUILD_DEVICE_BYTES")
    item = EC.first_item_offset(full)
    assert refused(EC.patched(full, item + 4, "<I", lambda v: P + 5), "is 0 or no pattern id") in ("loader", "seed")
    assert refused(EC.patched(full, item + 4, "<I", lambda v: 0), "a value of its tables is 0 or no pattern id") == "seed"
    hdr = EC.pattern_header_offsets(full)
    assert len(hdr) == P
    assert refused(EC.patched(full, hdr[1], "<q", lambda v: v + 1), r"tables hold \d+ k-mers, the num_kmers of its patterns add up to \d+") == "seed"
    fields = BC.pattern_headers(BC.split_db(full)["patterns_raw"])
    q = next(p for p in range(2, P) if fields[p][0] >= 1)           # a k-mer moves from pattern q to pattern 1: the totals still agree
    moved = EC.patched(EC.patched(full, hdr[1], "<q", lambda v: v + 1), hdr[q], "<q", lambda v: v - 1)
    assert refused(moved, "differ from the pattern's num_kmers") == "seed"
    assert refused(EC.patched(full, hdr[2] + 8, "<q", lambda v: 2), "parent_id is not below its own id") == "seed"
    assert refused(EC.patched(full, hdr[1] + 24, "<I", lambda v: 1 << 20), "sample ids are not strictly ascending below the number of samples") == "seed"
    # a good file seeds, extends and finishes in the same process afterwards
    got, _ = EC.extend_file(K, good, [], [], str(tmp_path / "again.db"))
    assert got == full
