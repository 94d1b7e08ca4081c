"""Helpers of tests/test_minhash.py: the bytes of a <sample>.minhash file assembled in Python, the oracle's words of a sample, the virus genomes
as the front-end sees them, and the batch that puts every edge of the device extractor's runs and tiles into one call.

Expected words never come from the code under test: they are the reference's recorded words (tests/golden/loader_extract.npz), the oracle's
extract_seq_alphabet (pinned to the reference by tests/test_loader_conformance.py), or a live oracle/_ref/ref_extract."""
import os
import struct

import numpy as np

import loader_cases as LC

SIGNATURE = 0xfedcba98                                              # MihashedInputFile::MINHASH_FORMAT_SIGNATURE (minhashed_input_file.h:44)
FRAMING = struct.calcsize("<IQ") + struct.calcsize("<Id")           # u32 signature, u64 count | u32 k, f64 fraction: no padding


def expected_file(words, k, fraction):
    """MihashedInputFile::store (minhashed_input_file.h:109-118): u32 signature, u64 count, the words, u32 k, f64 fraction, little-endian"""
    w = np.ascontiguousarray(words, dtype="<u8")
    return struct.pack("<IQ", SIGNATURE, w.size) + w.tobytes() + struct.pack("<Id", k, fraction)


def fasta_records(path):
    """the sequences of a FASTA file, line ends removed (genome_input_file.h:287-337)"""
    raw = open(path, "rb").read()
    return [b"".join(chunk.split(b"\n")[1:]).replace(b"\r", b"") for chunk in raw.split(b">")[1:]]


def oracle_words(O, records, k, alphabet, fraction, start=0.0):
    """sort-unique of the oracle's words of every record of a sample"""
    parts = [O.extract_seq_alphabet(r, k, alphabet, fraction, start) for r in records if len(r)]
    return LC.sort_unique(np.concatenate(parts + [np.zeros(0, np.uint64)]))


def sample_words(O, text, k, alphabet, fraction, start=0.0):
    """the same for a sample given as the device entry takes it: records joined by '\\n'"""
    return oracle_words(O, text.split(b"\n"), k, alphabet, fraction, start)


def virus_entries(golden_dir, list_name="virus.seqs.list"):
    with open(os.path.join(golden_dir, list_name)) as f:
        return [ln.strip() for ln in f if ln.strip()]


def link_virus_data(golden_dir, root):
    """<root>/test/virus/data/<name>.fasta -> the unpacked genomes: the list entries (./test/virus/data/<name>) resolve with cwd = root and
    the <entry>.minhash files a test writes stay in its own directory"""
    src = os.path.join(golden_dir, "test", "virus", "data")
    dst = os.path.join(root, "test", "virus", "data")
    os.makedirs(dst)
    for fn in os.listdir(src):
        if not fn.endswith(".minhash"):
            os.symlink(os.path.join(src, fn), os.path.join(dst, fn))
    return root


def dropped_homopolymer(O, alphabet, k, fraction, start):
    """a letter whose homopolymer k-mer falls OUTSIDE the window (decided by the oracle): a tile of it keeps nothing"""
    for g in LC.GROUPS[alphabet].split(","):
        letter = g[-1].encode()
        if O.extract_seq_alphabet(letter * k, k, alphabet, 1.0, 0.0).size == 1 and O.extract_seq_alphabet(letter * k, k, alphabet, fraction, start).size == 0:
            return letter
    raise AssertionError("every homopolymer of %s, k = %d lies inside the window (%g, %g)" % (alphabet, k, fraction, start))


def edge_batch(alphabet, k, R, T, quiet_letter):
    """One batch whose flat text (every sample followed by one separator byte, the first sample at position 0) puts every edge of the extractor
    on a run (R positions of a thread) or tile (T positions of a workgroup) boundary.  Returns (texts, notes): notes name what each sample is
    for and are checked here against the positions they claim."""
    rng = np.random.default_rng([20261018, LC.ALPHABETS.index(alphabet), k, R, T])
    bad = b"N" if alphabet.startswith("nt") else b"X"
    rnd = lambda n: bytearray(LC.random_text(rng, alphabet, n, lower_rate=0.2))      # noqa: E731
    texts, notes = [], []
    pos = [0]                                                       # flat position of the next sample's first symbol

    def add(t, note):
        texts.append(bytes(t))
        notes.append((note, pos[0], len(t)))
        pos[0] += len(t) + 1

    def index_at(residue, modulus, least):
        """the first index i >= least of the NEXT sample with (start + i) % modulus == residue"""
        i = (residue - pos[0]) % modulus
        while i < least:
            i += modulus
        return i

    add(b"", "empty first sample")
    add(rnd(k - 1), "shorter than k")
    for n, name in ((R - 1, "R-1"), (R, "R"), (R + 1, "R+1")):
        add(rnd(n), "length " + name)
        add(b"", "empty")
    # an invalid symbol at the last position of a run, and one at the first position of the next run
    for residue, name in ((R - 1, "invalid at the last position of a run"), (0, "invalid at the first position of a run")):
        i = index_at(residue, R, k + 3)
        t = rnd(i + 2 * k + 5)
        t[i] = bad[0]
        add(t, name)
        assert (notes[-1][1] + i) % R == residue
    # a record boundary at a run edge
    i = index_at(R - 1, R, k + 3)
    t = rnd(i + 2 * k + 5)
    t[i] = ord("\n")
    add(t, "record boundary at a run edge")
    # a sample boundary in the middle of a run: the separator behind this sample sits at residue R / 2
    n = index_at(R // 2, R, k + 2)
    add(rnd(n), "sample boundary in the middle of a run")
    assert (notes[-1][1] + n) % R == R // 2
    add(rnd(2 * k + 1), "the sample behind it")
    # a sample boundary exactly at a tile edge: the separator is the last position of a tile, the next sample starts a tile
    n = index_at(T - 1, T, k + 2)
    add(rnd(n), "sample boundary at a tile edge")
    assert (notes[-1][1] + n) % T == T - 1 and pos[0] % T == 0
    for n, name in ((T - 1, "T-1"), (T, "T"), (T + 1, "T+1"), (T + k - 1, "T+k-1")):
        add(rnd(n), "length " + name)
    # a record boundary at a tile edge (the first position of a tile), inside a sample that spans it
    i = index_at(0, T, k + 3)
    t = rnd(i + 3 * k)
    t[i] = ord("\n")
    add(t, "record boundary at a tile edge")
    assert (notes[-1][1] + i) % T == 0
    # tiles in which nothing is kept: a homopolymer whose word is outside the window (all of it kept as ONE word where there is no filter),
    # and a stretch of symbols outside the alphabet
    add(quiet_letter * (2 * T + R + 3), "homopolymer over whole tiles")
    add(bad * (T + 5), "no symbol of the alphabet over a whole tile")
    add(rnd(3 * k), "after the quiet tiles")
    add(b"", "empty last sample")
    return texts, notes
