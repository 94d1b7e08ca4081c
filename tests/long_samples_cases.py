"""Inputs of tests/test_long_samples.py: pairs of ascending lists that put every edge of the merge-union's tiles into a call, texts whose
section cuts fall on every kind of position, and the piece / section counts of a batch restated from the lengths alone.

Expected results never come from the code under test: numpy.union1d for the union, the oracle's extractor (minhash_cases.sample_words) or the
host extractor for the words of a sample, the reference's golden tables for the command line."""
import numpy as np

import loader_cases as LC

U64 = np.uint64
TOP = 1 << 63


def _merged_sources(a, b):
    """source (0 = A, 1 = B) of every position of the merged order, a word of A in front of an equal word of B"""
    words = np.concatenate([a, b])
    src = np.concatenate([np.zeros(a.size, np.int8), np.ones(b.size, np.int8)])
    return src[np.argsort(words, kind="stable")], np.sort(words, kind="stable")


def _from_merged(values, sources):
    v, s = np.asarray(values, U64), np.asarray(sources)
    return v[s == 0], v[s == 1]


def straddling_pairs(T, borders, n_tiles):
    """n_tiles * T merged words, sources alternating, where for every border d of `borders` the word at merged position d - 1 comes from A and the
    EQUAL word at position d from B: the duplicate's A-side lies in the tile in front of the border.  Checked against the merged order."""
    n = n_tiles * T
    step = np.ones(n, np.int64)
    step[list(borders)] = 0
    values = (np.cumsum(step) * 3 + 5).astype(U64)
    sources = (np.arange(n) + 1) % 2 if (borders[0] - 1) % 2 else np.arange(n) % 2      # position d - 1 is A's
    a, b = _from_merged(values, sources)
    src, merged = _merged_sources(a, b)
    for d in borders:
        assert src[d - 1] == 0 and src[d] == 1 and merged[d - 1] == merged[d], d
    return a, b


def union_cases(T, big=1000000):
    """{name: (A, B)}: strictly ascending uint64 arrays.  T = merged words per tile of the kernel (kmdb_sorted_union_geometry); big = words a
    side of the random case (the test's parameter list is made with a small one: the names do not depend on it)."""
    rng = np.random.default_rng(20261020)

    def asc(n, lo=0, hi=1 << 62):
        w = np.unique(rng.integers(lo, hi, size=n + n // 8 + 8, dtype=np.uint64))
        assert w.size >= n
        return np.sort(rng.choice(w, n, replace=False))

    empty = np.zeros(0, U64)
    c = {}
    c["0+0"] = (empty, empty)
    c["0+n"] = (empty, asc(777))
    c["n+0"] = (asc(777), empty)
    c["1+1 equal"] = (np.array([42], U64), np.array([42], U64))
    c["1+1 unequal, A first"] = (np.array([41], U64), np.array([42], U64))
    c["1+1 unequal, B first"] = (np.array([43], U64), np.array([42], U64))
    same = asc(T + 300)
    c["identical lists"] = (same, same.copy())
    inter = np.arange(2 * T + 11, dtype=U64) * U64(7)
    c["disjoint, interleaved"] = (inter[0::2].copy(), inter[1::2].copy())
    c["all of B below A"] = (asc(T + 5, 1 << 40, 1 << 41), asc(T // 2 + 3, 0, 1 << 39))
    c["all of B above A"] = (asc(T + 5, 0, 1 << 39), asc(T // 2 + 3, 1 << 40, 1 << 41))
    for tiles in (1, 2):
        for delta in (-1, 0, 1):
            n = tiles * T + delta
            na = n // 3
            pool = asc(n)                                           # n distinct words: merged length = union length = n
            pick = np.zeros(n, bool)
            pick[rng.choice(n, na, replace=False)] = True
            c["merged length %dT%+d" % (tiles, delta)] = (pool[pick], pool[~pick])
    # a quarter of the words common: the merged length is the tiles' edge, the union is shorter
    for delta in (-1, 0, 1):
        n = 2 * T + delta
        common = asc(n // 4)
        rest = np.setdiff1d(asc(n), common)[: n - 2 * common.size]
        a = np.union1d(common, rest[0::2])
        b = np.union1d(common, rest[1::2])
        assert a.size + b.size == n
        c["merged length 2T%+d, a quarter common" % delta] = (a, b)
    c["a duplicate pair straddling both borders of three tiles"] = straddling_pairs(T, (T, 2 * T), 3)
    # every border of a longer case, and pairs that end / begin exactly at a border (A at d - 2, B at d - 1; A at d, B at d + 1)
    c["a duplicate pair straddling every border of five tiles"] = straddling_pairs(T, tuple(T * t for t in range(1, 5)), 5)
    c["duplicate pairs that end at a border"] = straddling_pairs(T, (T - 1, 2 * T - 1), 3)
    c["duplicate pairs that begin at a border"] = straddling_pairs(T, (T + 1, 2 * T + 1), 3)
    # a run of ties: every word of B equals a word of A and one word of A alone in front shifts the pairs, so that EVERY diagonal (the tiles'
    # and, T being a multiple of the thread's share, the threads' too) falls between the two words of a pair
    run = asc(2 * T + 100, 1000, 1 << 50)
    a = np.concatenate([np.array([7], U64), run])
    src, _ = _merged_sources(a, run)
    assert src[T - 1] == 0 and src[T] == 1 and src[2 * T - 1] == 0 and src[2 * T] == 1
    c["partition diagonals inside a run of ties"] = (a, run.copy())
    # unsigned order: words on both sides of 2^63 in both lists, some common
    low, high = asc(T, 0, TOP), asc(T, TOP, (1 << 64) - 1)
    mixed = np.concatenate([low, high])
    c["words >= 2^63 on both sides"] = (mixed[0::2].copy(), np.union1d(mixed[1::2], mixed[0::16]))
    c["only words >= 2^63"] = (high[0::3].copy(), high[1::2].copy())
    c["the largest word in both"] = (np.array([0, TOP, (1 << 64) - 1], U64), np.array([1, (1 << 64) - 1], U64))
    # 10^6 random words a side, 30 % of B taken from A
    a = asc(big, 0, (1 << 64) - 1)
    b = np.union1d(rng.choice(a, big * 3 // 10, replace=False), asc(big - big * 3 // 10, 0, (1 << 64) - 1))
    c["1e6 random words, 30 % overlap"] = (a, b)
    for name, (x, y) in c.items():
        for w in (x, y):
            assert w.dtype == U64 and (w.size < 2 or bool(np.all(w[1:] > w[:-1]))), name
    return c


# ---- sections ------------------------------------------------------------------------------------------------------------------------
MAX_SAMPLE = 1000                                                   # KMDB_MINHASH_MAX_SAMPLE_BASES of the section tests
BUDGETS = (700, 997, 4096 + 5)                                      # KMDB_MINHASH_BASES_PER_PIECE
LENGTHS = (1001, 2500, 9000)
CONFIGS = (("nt", 5), ("nt", 18), ("nt", 20), ("nt", 31), ("nt-preserve", 18), ("aa", 6))
WINDOWS = ((1.0, 0.0), (0.3, 0.1))
PIECE_LIMIT = (1 << 31) - 2


def section_text(alphabet, k, n):
    """n bytes: random symbols, a few bytes outside the alphabet and two record ends"""
    rng = np.random.default_rng([20261020, LC.ALPHABETS.index(alphabet), k, n])
    t = bytearray(LC.random_text(rng, alphabet, n, invalid_rate=0.002, lower_rate=0.1))
    for at in rng.choice(n, 2, replace=False):
        t[at] = ord("\n")
    return bytes(t)


def sections_of(length, budget, max_sample=MAX_SAMPLE):
    """sections a sample is extracted in; 0: it is no long sample"""
    if length <= max_sample and length < PIECE_LIMIT:
        return 0
    step = min(budget, PIECE_LIMIT - 1)
    return -(-length // step)


def pieces_of(lengths, budget, max_sample=MAX_SAMPLE):
    """(pieces, long samples, sections) of a batch, from the lengths alone: the samples between two long ones are cut where the accumulated bytes
    (every sample counts one more, its separator) would pass the budget, a sample beyond the budget goes alone, a section is a piece"""
    pieces = longs = sections = 0
    acc = None                                                      # bytes of the open piece
    for n in lengths:
        s = sections_of(n, budget, max_sample)
        if s:
            pieces += s
            longs += 1
            sections += s
            acc = None
        elif acc is None or acc + n + 1 > budget:
            pieces += 1
            acc = n + 1
        else:
            acc += n + 1
    return pieces, longs, sections


def crafted_cuts(k, budget):
    """[(what, text)] for ONE alphabet (nt) and budget: the first cut lies between positions budget - 1 and budget.  Each text is checked here
    against the position it claims."""
    rng = np.random.default_rng([20261020, k, budget])
    rnd = lambda n: bytearray(LC.random_text(rng, "nt", n))         # noqa: E731
    c = budget                                                      # the first position of the second section
    n = 2 * budget + 300
    out = []

    def put(what, edits, length=n):
        t = rnd(length)
        for at, byte in edits:
            t[at] = ord(byte)
        out.append((what, bytes(t)))

    put("a cut inside a valid run", [])
    assert all(ch in b"ACGTU" for ch in out[-1][1][c - 40: c + 40])
    put("a cut one symbol after an invalid byte", [(c - 2, "N")])
    put("a cut right after an invalid byte", [(c - 1, "N")])
    put("a cut right before an invalid byte", [(c, "N")])
    put("a cut one symbol before an invalid byte", [(c + 1, "N")])
    put("a cut behind the newline between two records", [(c - 1, "\n")])
    put("a cut in front of the newline between two records", [(c, "\n")])
    put("a cut k-1 symbols after a record start", [(c - k, "\n")])              # the record's symbols c-k+1 .. c-1 lie in front of the cut
    put("a cut k symbols after a record start", [(c - k - 1, "\n")])
    put("a cut k-2 symbols after a record start", [(c - k + 1, "\n")])
    put("a last section of 1 symbol", [], 2 * budget + 1)
    out.append(("only invalid bytes", b"N" * (2 * budget + 5)))
    out.append(("one word repeated across the cuts", bytes(rnd(k) * (3 * budget // k + 1))))
    return out
