"""Inputs and references of test_gamma_conformance.py: an Elias-gamma coder of its own, the case families that put every code length at
every bit offset in front of the engine's stream readers, and a census that proves on the host what the families hold.  Host only.

The engine has two gamma readers ("The stream readers"): RunCursor32 (32-bit units, all2all's decode kernel, two launches) and
GammaCursor, 64 bit — <2>, three words: the v1 kernels, the upload's estimates, new2all's checkpoints; <1>, two words: new2all (run index,
walk, queued lists) and db2db (list store and root-path climb).  A reader that is one bit off at one alignment must fail here.

The coder (encode / decode) is plain Python on big integers: a stream is ONE int, most significant bit first, cut into uint64 words of
which the first holds the first 64 bits (reference src/elias_gamma.h:104-128); a value d of L bits is L - 1 ones, a zero and the L - 1 low
bits of d; a pattern's stream is padded to a multiple of 128 bits (src/pattern.h:79-81).  It shares no code with synth.gamma_encode_patterns,
the encoder of every other test: test_gamma_conformance.py holds the two against each other.

A case list is its deltas; the first id is given when the forest is built.  Every list goes into its forest twice: as a root, and under a parent of three ids (PARENT_IDS).
Alignment is made INSIDE a list, by a prefix of t codes of known length, never by a filler node: how the upload packs the streams does
not matter, over t = 0 .. 63 the code under test meets every bit offset of a 64-bit word and of a 32-bit unit wherever its stream starts.

Limits of the coverage, stated rather than pretended:
  * RunCursor32 reads codes of up to 39 bits, all2all serves at most 2^17 samples' worth of matrix in memory (131 072 samples are a
    34 GB matrix): deltas of 2^17 and more — codes of 35 to 39 bits — reach GammaCursor<1> and GammaCursor<2> (collection D), never
    RunCursor32.  Its 64-bit side path is exercised by the 33-bit codes of collection C only.
  * A delta cannot exceed N - 1: the last value of the longest code length of a collection, 2^(j + 1) - 1, is lowered to what the id range
    leaves behind the prefix and the tail (it keeps its code length), and the tail's 2^j is halved until it fits.  One list without a
    prefix holds the largest delta of the collection, N - 1.
  * In collection C (65 600 samples) a delta of 65 535 and more leaves at most 64 ids for prefix and tail: the 31 / 33-bit pair is placed
    at every offset of a 32-bit unit behind zeros and at 20 and more offsets at the head of a step, not at all 64 of a word.
"""
import functools

import numpy as np

import variant_cases as V

M64 = (1 << 64) - 1
PARENT_IDS = (0, 2, 3)
CHECKPOINT_LENGTHS = (32, 33, 64, 65, 96, 97, 200)
CHECKPOINT_POSITIONS = (31, 32, 33, 63, 64, 65)


# ------------------------------------------------------------------------------------------------------------------------------------
# the coder
# ------------------------------------------------------------------------------------------------------------------------------------
def code_of(d):
    """(code, length) of one value d >= 1"""
    L = int(d).bit_length()
    assert L >= 1
    return (((1 << (L - 1)) - 1) << L) | (int(d) - (1 << (L - 1))), 2 * L - 1


def encode(deltas):
    """-> (uint64 words, number of stream bits): the codes one after the other from the top bit of word 0, padded to 128 bits"""
    v = n = 0
    for d in deltas:
        c, ln = code_of(d)
        v = (v << ln) | c
        n += ln
    nw = (n + 127) // 128 * 2
    v <<= nw * 64 - n
    return [(v >> (64 * (nw - 1 - i))) & M64 for i in range(nw)], n


def decode_codes(words, nbits, l):
    """the l - 1 codes of a stream: [(value, first bit, length, "0" codes directly before it)]"""
    s = "".join(format(int(w), "064b") for w in words)
    out, pos, z = [], 0, 0
    for _ in range(max(l - 1, 0)):
        ones = s.index("0", pos) - pos
        ln = 2 * ones + 1
        d = (1 << ones) | int(s[pos + ones: pos + ln], 2)
        out.append((d, pos, ln, z))
        z = z + 1 if d == 1 else 0
        pos += ln
    assert pos == nbits and "1" not in s[pos:], "the stream ends where num_bits says, zero padding behind it"
    return out


def decode(words, nbits, l, last):
    """the l ids of a list (src/pattern.cpp:99-109: l - 1 deltas in append order, the first id = last - their sum)"""
    if l == 0:
        return []
    d = [c[0] for c in decode_codes(words, nbits, l)]
    ids = [last - sum(d)]
    for x in d:
        ids.append(ids[-1] + x)
    return ids


# ------------------------------------------------------------------------------------------------------------------------------------
# case families: lists as (tag, deltas)
# ------------------------------------------------------------------------------------------------------------------------------------
def D_of(j):
    """the first and the last value of code length 2 j + 1"""
    return (1 << j, (2 << j) - 1)


def _fill_bits(nbits, k=0):
    """deltas below 8 whose codes take exactly nbits bits, mostly 5-bit codes (deltas 4 .. 7 in turn)"""
    out = [4 + (i + k) % 4 for i in range(nbits // 5)]
    out += {0: [], 1: [1], 2: [1, 1], 3: [2], 4: [3, 1]}[nbits % 5]
    return out


def _gap(nbits, k=0):
    """deltas of 1 and 2 whose codes take exactly nbits bits: twos and ones in turn"""
    out = []
    while nbits >= 4:
        out += [2, 1]
        nbits -= 4
    return out + {0: [], 1: [1], 2: [1, 1], 3: [2]}[nbits]


class _Builder:
    """collects case lists for a collection of N samples; a list that the id range cannot hold is counted, not built"""

    def __init__(self, N):
        self.N, self.lists, self.dropped = N, [], 0

    def room(self):
        return self.N - 1 - (PARENT_IDS[-1] + 3)              # what the deltas of a list may add up to, as a root or under the parent

    def add(self, tag, deltas):
        if sum(deltas) > self.room():
            self.dropped += 1
            return False
        self.lists.append((tag, [int(d) for d in deltas]))
        return True

    def long_code(self, prefix_sum, j, hi, tail_ones=2):
        """(delta of code length 2 j + 1, second delta of the tail): 2^j or 2^(j + 1) - 1 and 2^j where the ids allow, else lowered"""
        room = self.room() - prefix_sum - tail_ones
        t2 = 1 << j
        while t2 > 1 and (1 << j) + t2 > room:
            t2 >>= 1
        d = min((2 << j) - 1 if hi else 1 << j, room - t2)
        return (d, t2) if d >= 1 << j else (None, None)

    # align(j, t, kind): a prefix of t codes — "ones": t bits, the code is met behind zeros; "twos": 3 t bits, met at the head of a step;
    # "ones40" (j <= 4): 40 ones more, a run of zeros longer than a 32-bit window — then the code, then the tail 1, 2^j, 1
    def align(self, js, ts_ones, ts_twos, values=(False, True)):
        for j in js:
            kinds = [("ones", t, [1] * t) for t in ts_ones] + [("twos", t, [2] * t) for t in ts_twos]
            if j <= 4:
                kinds += [("ones40", t, [1] * (t + 40)) for t in ts_ones]
            for kind, t, prefix in kinds:
                for hi in values:
                    d, t2 = self.long_code(sum(prefix), j, hi)
                    if d is None:
                        self.dropped += 1
                        continue
                    self.add(("align", j, t, kind, hi), prefix + [d, 1, t2, 1])

    def align_delta(self, d, ts_ones, ts_twos):
        """one given delta behind the same prefixes, tail 1, 1 (collection C: the deltas either side of 65 536 leave no room for more)"""
        for kind, t, prefix in [("ones", t, [1] * t) for t in ts_ones] + [("twos", t, [2] * t) for t in ts_twos]:
            self.add(("align", d, t, kind, None), prefix + [d, 1, 1])

    def bits128(self, last_deltas):
        """at most 48 ids and a stream of exactly 127 / 128 / 129 bits, the last code of each given length; 49 ids below 128 bits"""
        for k, last in enumerate(last_deltas):
            for total in (127, 128, 129):
                deltas = _fill_bits(total - code_of(last)[1], k) + [last]
                assert len(deltas) + 1 <= 48
                self.add(("bits128", total, last), deltas)
        self.add(("ids49", 48), [1] * 48)
        self.add(("ids49", 84), [1, 1, 2, 1, 1, 2, 1, 2] * 6)

    def units(self, jmax):
        """long-launch lists: 200 .. 600 ids, 18 .. 31 units in A; the deltas run through D(1 .. jmax) from different starts, 1 where the
        ids run out; and lists whose longest code starts o bits before stream bit 448 k (the reload of the long launch: every 14 units)"""
        Dall = [d for j in range(1, jmax + 1) for d in D_of(j)]
        for n, L in enumerate((200, 333, 450, 600)):
            deltas, k, left = [], 5 * n, self.room() - (L - 1)              # left: what the deltas may exceed 1 by, in all
            while len(deltas) < L - 1:
                d = Dall[k % len(Dall)] if len(deltas) % 3 == 0 else 1      # two zeros between the codes keep the list inside 40 units
                k += len(deltas) % 3 == 0
                if d - 1 > left // 2:
                    d = 1
                left -= d - 1
                deltas.append(d)
            self.add(("units", L), deltas)
        for o in range(1, 64, 4):
            d1, _ = self.long_code(450, jmax, False, 0)
            if d1 is None:
                self.dropped += 1
                continue
            first = _gap(448 - o)
            second = _gap(448 - code_of(d1)[1])
            d2 = min(1 << (jmax - 1), self.room() - sum(first) - sum(second) - d1 - 30)
            if d2 < 2:
                self.dropped += 1
                continue
            self.add(("reload", o), first + [d1] + second + [d2] + [1, 2] * 10)

    def checkpoints(self, jmax):
        """a code of the longest length directly before, on and directly after every 32nd id of a list; 1 (then 2) everywhere else"""
        for L in CHECKPOINT_LENGTHS:
            for p in CHECKPOINT_POSITIONS:
                if p >= L:
                    continue
                for fill in (1, 2):
                    for hi in (False, True):
                        d, _ = self.long_code(fill * (L - 2), jmax, hi, 0)
                        if d is None:
                            self.dropped += 1
                            continue
                        deltas = [fill] * (L - 1)
                        deltas[p - 1] = d                                   # the delta that leads to id p of the list
                        self.add(("checkpoint", L, p, fill, hi), deltas)

    def forest(self, extra_roots=()):
        """every list as a root (first id 0 .. 2) and under the parent (first id behind its last); extra_roots: [(tag, ids)] as they are"""
        F = V._Forest()
        par = F.add(PARENT_IDS, -1, 3)
        tags = [None, ("parent",)]
        for n, (tag, deltas) in enumerate(self.lists):
            for under in (False, True):
                first = PARENT_IDS[-1] + 1 + n % 3 if under else n % 3
                ids = np.concatenate([[first], first + np.cumsum(deltas)]).astype(np.int64)
                assert ids[-1] < self.N
                F.add(ids, par if under else -1, 1 + (n + under) % 5)
                tags.append(tag + ("under" if under else "root",))
        for tag, ids in extra_roots:
            F.add(ids, -1, 2)
            tags.append(tag + ("root",))
        return F.pat(), tags


def run_lists(N, max_len):
    """new2all's run index: lists that are one run of consecutive ids of max_len - 1 .. 2 max_len + 1 ids (a run of more than max_len ids is
    stored as several), from id 0 and up to id N - 1, and two runs a delta of 2 apart.  [(tag, ids)]"""
    out = []
    for n in (max_len - 1, max_len, max_len + 1, 2 * max_len + 1):
        if n > N:
            continue
        out.append((("run", n, "from 0"), np.arange(0, n)))
        out.append((("run", n, "to N - 1"), np.arange(N - n, N)))
        if n + 7 < N:
            out.append((("run", n, "inside"), np.arange(7, 7 + n)))
    a = min(max_len, (N - 2) // 2)
    out.append((("two runs", a, a), np.concatenate([np.arange(0, a), np.arange(a + 1, 2 * a + 1)])))
    b = min(max_len + 1, N - 41)                                            # (the second run is split where the ids hold max_len + 1 of them)
    out.append((("two runs", 40, b), np.concatenate([np.arange(0, 40), np.arange(41, 41 + b)])))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# collections
# ------------------------------------------------------------------------------------------------------------------------------------
ODD, EVEN = tuple(range(1, 64, 2)), tuple(range(2, 65, 2))
SIZES = {"A": 4096, "B": 65535, "C": 65600, "D": (1 << 19) + (1 << 11), "R16": 65536}
JS = {"A": range(1, 12), "B": range(12, 16), "D": range(16, 20)}


@functools.lru_cache(maxsize=None)
def collection(name):
    """(forest, tag per pattern, N).  A: every t, both kinds (ones: t = 1 .. 64 — t = 0 is the twos' t = 0, and the offset 0 behind zeros
    needs 64 of them); B, D: ones with even t, twos with odd t (3 t mod 64 runs through the odd offsets).  R16: the run lists at 65 536
    samples (new2all keeps 16-bit starts up to there)."""
    N = SIZES[name]
    b = _Builder(N)
    extra = []
    if name == "A":
        b.align(JS["A"], range(1, 65), range(0, 64))
        b.bits128([1, (1 << 11) + 5])
        b.units(11)
        b.checkpoints(11)
        # queued lists whose last run ends at id N - 1 and at id N - 2: the difference form of the walk leaves out its -H behind the former only
        extra = [(("run end", N - 1), np.arange(N - 40, N)), (("run end", N - 2), np.arange(N - 41, N - 1)),
                 (("run end", N - 2, "two runs"), np.concatenate([np.arange(N - 90, N - 50), np.arange(N - 41, N - 1)]))]
    elif name == "B":
        b.align(JS["B"], EVEN, ODD)
        b.bits128([1, (1 << 15) + 77])
        b.checkpoints(15)
    elif name == "C":
        for d in (65535, 65536, 65537):
            b.align_delta(d, range(1, 60), range(0, 30))
        b.align_delta(65590, range(1, 4), range(0, 2))
        b.bits128([1, 32768 + 5])
        b.add(("bits128", 33, 65536), [65536])
    elif name == "D":
        b.align(JS["D"], EVEN, ODD)
        b.bits128([1, (1 << 15) + 77, (1 << 16) + 3, (1 << 19) + 1])
        b.checkpoints(19)
        extra = run_lists(N, 4095)
    elif name == "R16":
        b.bits128([1])
        extra = run_lists(N, 65535)
    extra.append((("largest delta",), np.array([0, N - 1])))
    pat, tags = b.forest(extra)
    return pat, tags, N


# ------------------------------------------------------------------------------------------------------------------------------------
# census
# ------------------------------------------------------------------------------------------------------------------------------------
def streams(arr):
    """per pattern (words, num_bits, l, last) of the view arrays of synth.to_view_arrays"""
    doff, nb, l, last, data = (arr[k] for k in ("data_offset", "num_bits", "num_local", "last_sample_id", "data"))
    for p in range(l.size):
        nw = (int(nb[p]) + 127) // 128 * 2
        yield data[int(doff[p]): int(doff[p]) + nw].tolist(), int(nb[p]), int(l[p]), int(last[p])


def census(arr, N, tags=None):
    """What the DECODED streams of a collection hold (the coder above reads the arrays that are uploaded: a mistake of the generators
    cannot make the census vacuous).  offsets[code length] = {"head": offsets mod 64 of such a code's first bit, counted from its stream's
    start, with no "0" code directly before it, "behind": with one or more}; bits_short: stream lengths among the lists of at most 48
    ids; lengths: list lengths; deltas; ids: smallest and largest; longest_zero_run.  With the tags of collection(): aligned — the same as
    offsets, but of the ONE code that an align list places behind its prefix, by its index in the decoded stream (the tails and the other
    families meet many offsets too: they must not stand in for a prefix that is missing)."""
    offsets, bits_short, lengths, deltas, aligned = {}, set(), set(), set(), {}
    p = -1
    lo, hi, zrun = N, -1, 0
    for words, nb, l, last in streams(arr):
        p += 1
        if l == 0:
            continue
        codes = decode_codes(words, nb, l)
        lengths.add(l)
        if tags is not None and tags[p][0] == "align":
            _, _, t, kind, _, _ = tags[p]
            d, pos, ln, z = codes[t + 40 * (kind == "ones40")]
            assert d > 1 and (z == 0) == (kind == "twos" or t + 40 * (kind == "ones40") == 0), tags[p]
            aligned.setdefault(ln, {"head": set(), "behind": set()})["behind" if z else "head"].add(pos % 64)
        if l <= 48:
            bits_short.add(nb)
        first = last - sum(c[0] for c in codes)
        assert 0 <= first and last < N
        lo, hi = min(lo, first), max(hi, last)
        for d, pos, ln, z in codes:
            zrun = max(zrun, z + (d == 1))
            if d > 1:
                deltas.add(d)
                offsets.setdefault(ln, {"head": set(), "behind": set()})["behind" if z else "head"].add(pos % 64)
    return {"offsets": offsets, "bits_short": bits_short, "lengths": lengths, "deltas": deltas, "ids": (lo, hi), "longest_zero_run": zrun,
            "aligned": aligned}


# ------------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------------
def sparse_definition(pat, N):
    """all2all from the definition as sorted (cell index int64, value uint32) pairs of the non-zero cells: cell (i, j), j < i, at
    i (i - 1) / 2 + j; uint32 sums wrap.  For collections whose matrix does not fit host arrays."""
    w = pat["num_kmers"].numpy()
    idx, val = [], []
    for p, full in enumerate(V.full_lists(pat)):
        if w[p] == 0 or full.size < 2:
            continue
        ii, jj = V._tril(full.size)
        idx.append(full[ii] * (full[ii] - 1) // 2 + full[jj])
        val.append(np.full(ii.size, w[p], dtype=np.uint64))
    idx, val = np.concatenate(idx), np.concatenate(val)
    cells, inv = np.unique(idx, return_inverse=True)
    sums = np.zeros(cells.size, dtype=np.uint64)
    np.add.at(sums, inv, val)
    sums = (sums & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    keep = sums != 0
    return cells[keep].astype(np.int64), sums[keep]


def with_dictionary(pat, seed):
    """a fabricated k-mer dictionary for a forest: pattern p holds 1 + p % 4 k-mers (neighbouring lists differ), the empty pattern none.
    -> (forest with these weights, sorted k-mers uint64, pattern of every k-mer, k-mers that are in no pattern)"""
    import torch
    P = int(pat["parent"].numel())
    w = 1 + np.arange(P, dtype=np.int64) % 4
    w[0] = 0
    rng = np.random.default_rng(seed)
    universe = rng.choice(1 << 36, size=int(w.sum()) + 500, replace=False).astype(np.uint64)
    kmers = np.sort(universe[: int(w.sum())])
    pids = rng.permutation(np.repeat(np.arange(P, dtype=np.int64), w))
    out = dict(pat)
    out["num_kmers"] = torch.from_numpy(w)
    return out, kmers, pids, universe[int(w.sum()):]


def column_forest():
    """the 64-sample column part of the db2db cases: roots, children and a chain; lists over both halves of the block"""
    F = V._Forest()
    a = F.add([0, 1, 2], -1, 1)
    b = F.add([5, 40], a, 1)
    F.add([41, 63], b, 1)
    F.add([63], a, 1)
    F.add(range(10, 30), -1, 1)
    F.add([31, 32], -1, 1)
    c = F.add([0], -1, 1)
    F.add(range(1, 64), c, 1)
    F.add([33, 35, 62], -1, 1)
    return F.pat()


def one2all_from_lists(pat, N, hit_pids):
    """a query's row from the lists: every hit k-mer adds 1 to every sample of its pattern's full list (uint32)"""
    hits = np.bincount(hit_pids, minlength=int(pat["parent"].numel()))
    row = np.zeros(N, dtype=np.uint32)
    for p, full in enumerate(V.full_lists(pat)):
        if hits[p]:
            row[full] += np.uint32(hits[p])
    return row


def db2db_from_lists(pat_r, Nr, pids_r, pat_c, Nc, pids_c):
    """the cell of two parts from the lists: shared k-mer i (pattern pids_r[i] of the rows, pids_c[i] of the columns) adds 1 to every
    pair (sample of the row pattern, sample of the column pattern)"""
    full_c = V.full_lists(pat_c)
    per = np.zeros((int(pat_r["parent"].numel()), Nc), dtype=np.uint32)
    for pr, pc in zip(pids_r.tolist(), pids_c.tolist()):
        per[pr, full_c[pc]] += 1
    out = np.zeros((Nr, Nc), dtype=np.uint32)
    for p, full in enumerate(V.full_lists(pat_r)):
        if per[p].any():
            out[full] += per[p]
    return out
