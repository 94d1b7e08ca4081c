"""Cases and helpers of tests/test_loader_conformance.py: the table of (alphabet, k, hash window, text) on which the three k-mer extractors of
this project — the oracle's (oracle/kmdb_oracle.c), the host loader (csrc/host_kmers.cpp) and the device loader (csrc/new2all.hip) — are
pinned to the words of the reference's own KmerHelper::extract (oracle/_ref/ref_extract), recorded in tests/golden/loader_extract.npz by
tests/golden/make_fixture_extract.py.  The texts are made here (a seeded generator), RECORDED in the fixture beside the reference's words, and
the tests read them from the fixture; test_fixture_texts_are_the_tables checks that both still agree.

Every text is 7-bit ASCII (the reference indexes its symbol table with a signed char; bytes >= 0x80 are out of scope)."""
import lzma
import os

import numpy as np

ALPHABETS = ("nt", "nt-preserve", "aa", "aa11_diamond", "aa12_mmseqs", "aa6_dayhoff")            # AlphabetType order (reference src/alphabet.h:10-18)
GROUPS = {"nt": "A,C,G,TU", "nt-preserve": "A,C,G,TU", "aa": "K,R,E,D,Q,N,C,G,H,I,L,V,M,F,Y,W,P,S,T,A", "aa11_diamond": "KREDQN,C,G,H,ILV,M,F,Y,W,P,STA",
          "aa12_mmseqs": "AST,C,DN,EQ,FY,G,H,IV,KR,LM,P,W", "aa6_dayhoff": "STPAG,NDEQ,HRK,MILV,FYW,C"}          # src/alphabet.h:79-86


def n_symbols(alphabet):
    return GROUPS[alphabet].count(",") + 1


def bits(alphabet):
    return int(np.ceil(np.log2(n_symbols(alphabet))))                # alphabet.h:37


def max_k(alphabet):
    return 64 // bits(alphabet) - 1                                  # alphabet.h:38


def widen(alphabet, k):
    return max(0, 8 - (bits(alphabet) * k - 32))                     # kmer_extract.h:37-45


def first_k_without_widening(alphabet):
    return next(k for k in range(1, max_k(alphabet) + 1) if bits(alphabet) * k - 32 >= 8)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
NT_K = (1, 4, 12, 15, 16, 17, 18, 19, 20, 22, 25, 28, 31)
PROTEIN = ("aa", "aa11_diamond", "aa12_mmseqs", "aa6_dayhoff")
# the device tests' protein databases (tests/golden/loader_<alphabet>_k<k>.db.xz): bits * k = 30, 36, 40 -> widening 10, 4, 0; 256 buckets each
GPU_PROTEIN = (("aa", 6), ("aa6_dayhoff", 12), ("aa11_diamond", 10))
CASES = [(a, k) for a in ("nt", "nt-preserve") for k in NT_K]
CASES += [(a, k) for a in PROTEIN for k in (1, 3, first_k_without_widening(a), max_k(a))]
CASES += [c for c in GPU_PROTEIN if c not in CASES]
WINDOWS = ((1.0, 0.0), (0.1, 0.0), (0.2, 0.4), (0.25, 0.5), (0.7, 0.3), (0.5, 0.5), (0.05, 0.95))       # (fraction, start); the last three end at 1
TOP_WINDOWS = (4, 5, 6)
# the device tests: bucket counts stay <= 4096 (k <= 22); k >= 26 needs >= 2^20 hash tables per database and is left to the CPU tests
GPU_CASES = [("nt", k) for k in (12, 15, 16, 17, 19, 20, 22)] + [("nt-preserve", 16), ("nt-preserve", 20)] + list(GPU_PROTEIN)
GPU_WINDOWS = (0, 2, 4)                                             # (1, 0), (0.2, 0.4), (0.7, 0.3)
GPU_N, GPU_CLADE, GPU_L, GPU_SEED = 48, 12, 3000, 20261018          # the synth collection of the nt device tests
PIECE = 120                                                         # symbols per own-genome piece
N_PIECES = 16                                                       # 8 clean + 8 noisy
PROTEIN_RECORDS, PROTEIN_RESIDUES = 24, 800
EDGE_LABELS = ("random", "invalid@0", "invalid@k-2", "invalid@k-1", "invalid@k", "invalid@last", "homopolymer0", "homopolymer1", "homopolymer2",
               "homopolymer-last", "palindrome", "len k-1", "len k", "len k+1", "interleaved repeat")
GPU_EDGE = (0, 3, 6, 10, 11, 12, 13, 14)                            # the edge texts that ride in every device batch (a third of 24)


def _letters(alphabet):
    """one list of letters per symbol, upper case"""
    return [list(g) for g in GROUPS[alphabet].split(",")]


def _invalid(alphabet):
    if alphabet.startswith("nt"):
        return list("NnRYXx-*.")                                    # ambiguity codes, gaps: no symbol of A,C,G,TU
    return list("BJOUXZbjouxz-*.")                                  # (U is a symbol of nt only)


def _rng(alphabet, k, salt):
    return np.random.default_rng([20261018, ALPHABETS.index(alphabet), k, salt])


def random_text(rng, alphabet, n, invalid_rate=0.0, lower_rate=0.0):
    """n letters: a uniform symbol, a uniform letter of its group (so nt gets U beside T), some in lower case, some outside the alphabet"""
    groups, bad = _letters(alphabet), _invalid(alphabet)
    out = []
    for _ in range(n):
        if rng.random() < invalid_rate:
            out.append(bad[rng.integers(len(bad))])
            continue
        g = groups[rng.integers(len(groups))]
        c = g[rng.integers(len(g))]
        out.append(c.lower() if rng.random() < lower_rate else c)
    return "".join(out).encode()


def _revcomp(t):
    return t[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def edge_texts(alphabet, k):
    """the 15 texts of EDGE_LABELS for one (alphabet, k)"""
    rng = _rng(alphabet, k, 1)
    groups = _letters(alphabet)
    bad = _invalid(alphabet)
    t = bytearray(random_text(rng, alphabet, 160, invalid_rate=1 / 40, lower_rate=0.3))
    t[50], t[101] = ord("U"), ord("u")                              # U in every random text: T's twin in nt, outside every protein alphabet
    texts = [bytes(t)]
    n = k + 8
    for at in (0, k - 2, k - 1, k, n - 1):                          # (k = 1: k - 2 falls on index 0 again)
        t = bytearray(random_text(rng, alphabet, n))
        t[max(at, 0)] = ord(bad[rng.integers(len(bad))])
        texts.append(bytes(t))
    for s in (0, 1, min(2, len(groups) - 1), len(groups) - 1):
        texts.append((groups[s][-1] * (k + 3)).encode())            # (nt: A, C, G and U)
    half = random_text(rng, alphabet, k + 2).upper().replace(b"U", b"T")
    texts.append(half + (_revcomp(half) if alphabet.startswith("nt") else half[::-1]))      # nt, even k: the middle window is its own reverse complement
    for n in (k - 1, k, k + 1):
        texts.append(random_text(rng, alphabet, n))
    # a k-mer, another that differs from it in the FIRST symbol only, and the first again, kept apart by letters outside the alphabet: where
    # the word is widened the two differ only above bit bits * k, so a sort that leaves the widening out of its width does not bring the two
    # copies of the first together (nt: the last letter A keeps both forward words below their reverse complements)
    rest = random_text(rng, alphabet, k - 1)[:max(k - 2, 0)] + (groups[0][-1].encode() if k > 1 else b"")
    x1, x2, sep = groups[0][-1].encode() + rest, groups[1][-1].encode() + rest, bad[0].encode()
    texts.append(x1 + sep + x2 + sep + x1)
    assert len(texts) == len(EDGE_LABELS) and all(max(t, default=0) < 0x80 for t in texts)
    return texts


def protein_records():
    """the first PROTEIN_RECORDS records of the reference's test/protein/aa_100x1000.fasta, the first PROTEIN_RESIDUES residues of each WITHOUT
    the '.' that follows every 8 letters in that file (with it no window longer than 8 is valid): (header, text)"""
    here = os.path.dirname(os.path.abspath(__file__))
    with lzma.open(os.path.join(here, "golden", "protein.aa_100x1000.fasta.xz")) as f:
        raw = f.read()
    recs = []
    for chunk in raw.split(b">")[1:1 + PROTEIN_RECORDS]:
        head, _, body = chunk.partition(b"\n")
        recs.append((head.split(b" ")[0].decode(), body.replace(b"\n", b"").replace(b"\r", b"").replace(b".", b"")[:PROTEIN_RESIDUES]))
    return recs


def genome_texts(alphabet):
    """the samples of the device tests' database as text: nt — the genomes of synth.CladeGenomes(GPU_N, GPU_CLADE, GPU_L, seed=GPU_SEED);
    protein — protein_records()"""
    if not alphabet.startswith("nt"):
        return [t for _, t in protein_records()]
    import importlib
    from _kmerdb_loader import import_kmerdb_amd
    import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    g = S.CladeGenomes(GPU_N, GPU_CLADE, GPU_L, seed=GPU_SEED)
    lut = np.frombuffer(b"ACGT", np.uint8)
    return [lut[g.sample(i).numpy()].tobytes() for i in range(GPU_N)]


def own_piece_meta(case):
    """(sample, clean?) of the N_PIECES own pieces of a case: 8 clean ones, then 8 with noise"""
    n = GPU_N if case[0].startswith("nt") else PROTEIN_RECORDS
    return [((j * 7 + 3 * (j // 8)) % n, j < N_PIECES // 2) for j in range(N_PIECES)]


def own_pieces(alphabet, k):
    """N_PIECES pieces of the samples' own texts, PIECE letters each: [(sample, clean?, text)].  Noise = substitutions at 2 %, one letter
    outside the alphabet, lower case at 30 %."""
    rng = _rng(alphabet, k, 2)
    gen = genome_texts(alphabet)
    groups = _letters(alphabet)
    bad = _invalid(alphabet)
    out = []
    for s, clean in own_piece_meta((alphabet, k)):
        at = int(rng.integers(0, len(gen[s]) - PIECE))
        t = bytearray(gen[s][at: at + PIECE])
        if not clean:
            for i in np.nonzero(rng.random(PIECE) < 0.02)[0]:
                g = groups[rng.integers(len(groups))]
                t[i] = ord(g[rng.integers(len(g))])
            t[int(rng.integers(PIECE))] = ord(bad[rng.integers(len(bad))])
            for i in np.nonzero(rng.random(PIECE) < 0.3)[0]:
                t[i] = ord(chr(t[i]).lower())
        out.append((s, clean, bytes(t)))
    return out


def gpu_batch(fx, case):
    """the 24 queries of one device call — 8 clean own pieces, 8 noisy ones, 8 edge texts — with the reference's words of every GPU window:
    (texts, {window index: [words per query]}, [(sample, clean?)] of the first 16)"""
    edge = fx.texts(case)
    texts = fx.pieces(case) + [edge[i] for i in GPU_EDGE]
    words = {}
    for wi in GPU_WINDOWS:
        ew = fx.words(case, wi)
        words[wi] = fx.piece_words(case, wi) + [ew[i] for i in GPU_EDGE]
    return texts, words, own_piece_meta(case)


# ---- the hash of MinHashFilter restated in numpy (src/filter.h:96-115): only to tie the recorded thresholds to the recorded words -------------
def minhash(words, k):
    with np.errstate(over="ignore"):
        u = np.uint64
        kd4 = u(-(-k // 4))

        def fmix(x):
            x = (x ^ (x >> u(33))) * u(0xff51afd7ed558ccd)
            x = (x ^ (x >> u(33))) * u(0xc4ceb9fe1a85ec53)
            return x ^ (x >> u(33))
        h = np.asarray(words, dtype=np.uint64) * u(0x87c37b91114253d5)
        h = (h << u(31)) | (h >> u(33))
        h = h * u(0x4cf5ad432745937f)
        h1 = (u(42) ^ h) ^ kd4
        h2 = np.full_like(h1, u(42) ^ kd4)
        h1 = h1 + h2
        h2 = h2 + h1
        h1, h2 = fmix(h1), fmix(h2)
        h1 = h1 + h2
        h2 = h2 + h1
        return h1 ^ h2


def sort_unique(words):
    return np.unique(np.asarray(words, dtype=np.uint64))


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loader_extract.npz")


def _split(flat, counts):
    ends = np.cumsum(counts)
    return [flat[e - c: e] for c, e in zip(counts, ends)]


class Fixture:
    """tests/golden/loader_extract.npz.  Arrays: `texts` / `text_len` — every text, case by case (CASES order: the 15 edge texts; then, for the
    GPU_CASES, the 16 own pieces); `words` / `word_cnt` — the reference's words in EXTRACTION order for every (case, window, text) in the same
    nesting (edge texts: all WINDOWS; own pieces: GPU_WINDOWS); `window_lo` / `window_hi` — the thresholds the reference's MinHashFilter held
    for every window (read from its own object)."""

    def __init__(self, path=FIXTURE):
        z = np.load(path)
        self.window_lo, self.window_hi = z["window_lo"], z["window_hi"]
        texts = [t.tobytes() for t in _split(z["texts"], z["text_len"])]
        words = _split(z["words"], z["word_cnt"])
        ne, ti, wi_ = len(EDGE_LABELS), 0, 0
        self._texts, self._words, self._pieces, self._piece_words = {}, {}, {}, {}
        for c in CASES:
            self._texts[c] = texts[ti: ti + ne]
            ti += ne
            for w in range(len(WINDOWS)):
                self._words[c, w] = words[wi_: wi_ + ne]
                wi_ += ne
        for c in GPU_CASES:
            self._pieces[c] = texts[ti: ti + N_PIECES]
            ti += N_PIECES
            for w in GPU_WINDOWS:
                self._piece_words[c, w] = words[wi_: wi_ + N_PIECES]
                wi_ += N_PIECES
        assert ti == len(texts) and wi_ == len(words), "the fixture does not have the shape of the case table: regenerate it (tests/golden/make_fixture_extract.py)"

    def texts(self, case):
        return list(self._texts[case])

    def words(self, case, window):
        return list(self._words[case, window])

    def pieces(self, case):
        return list(self._pieces[case])

    def piece_words(self, case, window):
        return list(self._piece_words[case, window])


def build_fixture_arrays(extract, window_of):
    """the arrays of the fixture from extract(alphabet, k, fraction, start, texts) -> [words] and window_of(fraction, start) -> (lo, hi)"""
    texts, words = [], []
    for a, k in CASES:
        et = edge_texts(a, k)
        texts += et
        for f, s in WINDOWS:
            words += extract(a, k, f, s, et)
    for a, k in GPU_CASES:
        pt = [t for _, _, t in own_pieces(a, k)]
        texts += pt
        for w in GPU_WINDOWS:
            words += extract(a, k, WINDOWS[w][0], WINDOWS[w][1], pt)
    win = [window_of(f, s) for f, s in WINDOWS]
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt).ravel() for x in xs] + [np.zeros(0, dt)])       # noqa: E731
    return {"texts": cat([np.frombuffer(t, np.uint8) for t in texts], np.uint8), "text_len": np.array([len(t) for t in texts], np.int32),
            "words": cat(words, np.uint64), "word_cnt": np.array([len(w) for w in words], np.int32),
            "window_lo": np.array([w[0] for w in win], np.uint64), "window_hi": np.array([w[1] for w in win], np.uint64)}
