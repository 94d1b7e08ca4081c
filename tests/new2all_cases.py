"""Inputs and references of test_new2all_conformance.py: databases whose hashtables are FABRICATED slot by slot (new2all looks k-mers up, it
never extracts them) and whose forests and query batches sit on the thresholds of csrc/hash_probe.h (kmdb_probe) and csrc/new2all.hip
(n2a_probe_kernel, the sort, n2a_walk_kernel, n2a_nodes_kernel), the definition of a query's row in numpy, and censuses that prove on
the host what the cases hold.  Host only: no GPU, no engine.

A case is a forest in the format of synth.build_patterns (see variant_cases.py), its Tables, and a batch of queries (sorted unique 40-bit
words: bucket = word >> 32, 256 buckets at k = 18, key = the low 32 bits).  The dictionary is READ BACK from the tables; num_kmers is the
bincount of its patterns.  Tables.check() asserts for every table a case writes that it is a valid hashmap_lp table: a power-of-two
capacity, an empty slot, no key twice, and every key reachable from its home slot without crossing an empty slot.

Group P (the probe; N = 48, 41 patterns):
  P1  capacities 1, 16, 1, 4, 2, 8, 2, 2, 16, ...: empty tables of one slot, tables of 2, tables of 4 / 8 / 16 at odd offsets (the scalar
      path) and at offsets = 2 mod 4 (the four-slot path, groups not sector-aligned); every home slot probed for an absent key
  P2  capacities 4, 16, 64 at offsets = 0 mod 4: keys at homes = 0 .. 3 mod 4, clusters across a group boundary and from the last slot
      to slots 0, 1, an empty slot BEFORE `first` in the home group of keys stored further on, a full home with an empty next slot
  P3  tables of 16 with 15 keys (and of 4 with 3) whose one empty slot e is = 0 mod 4: a key with home e + 1 stored at e - 1 (found in the
      last group before the revisit), absent keys with homes e + 1 .. e + 3 (they end at e on the fifth round)
  P4  key 0 (the key of an empty slot) present at home, present behind another key, and absent where its home slot is empty; one 32-bit
      key in three buckets under three patterns; a word whose bucket is >= 256 (the oracle takes it: a miss)
Group W (the walk):
  W1   N = 128, root subtrees that are chains of 1 / 2 / 3 nodes of 33 local ids (twins: 32): queries whose hits make one workgroup
       file 1023, 1024, 1025 and 1500 long lists (N2_QCAP = 1024), at 512 and at 1024 threads
  W2   queries of 511 / 512 / 513 / 1024 / 1025 distinct hit patterns, 1 .. 300 k-mers per pattern; a root whose subtree holds 2016 hits
       of one query, a hit that is the ancestor of the next 600 hits, hits with hit descendants in the last thread of a workgroup
  W3a / W3b   P = 1023 / 1024 patterns; 613 queries: 600 of one hit, five empty and five all-miss (first, inside, before the last), one
       query three times; the last query hits the last DFS node
  W4_<N>  N = 11008 / 11009 / 9984 / 9985: either side of the LDS limit of the per-query histogram at 512 / 1024 threads (lds_limits()
       derives them from the expression in n2a_run); clade-like lists, queued lists whose runs end at N - 1 and at N - 2
  W5   N = 131200: roots of 65534 / 65535 / 65536 non-adjacent ids (as many runs: the run count of n2a_nodes_kernel clips at 0xFFFF) and
       of 70 000 consecutive ids (l clipped, 18 runs), a child and a grandchild each; queries hit the grandchildren"""
import functools
import os
import re

import numpy as np

import variant_cases as V
from build_cases import fmix32, keys_with_home
from db2db_cases import dfs_index, forest_of

K_LEN = 18
N_BUCKETS = 256
EMPTY_VAL = 0x7fffffff
EMPTY = np.uint64(EMPTY_VAL) << np.uint64(32)
CSRC = os.path.join(V.ROOT, "kmer-db_amd", "csrc")
CK_IDS = 32                                             # KMDB_CK_IDS (engine_internal.h): a longer local list goes to the queue
QCAP = 1024                                             # N2_QCAP
THREADS = (512, 1024)


# ------------------------------------------------------------------------------------------------------------------------------------
# the engine's constants, read from the source
# ------------------------------------------------------------------------------------------------------------------------------------
_LDS_TEXT = "const bool lds_hist = N * 4 + qcap * 16 + threads * 8 + 1024 <= 64 * 1024;"


@functools.lru_cache(maxsize=None)
def lds_limits():
    """{threads: the largest N whose histogram n2a_run keeps in LDS}, from the expression in new2all.hip (and KMDB_CK_IDS, N2_QCAP as this
    module restates them): a change of the static LDS moves W4 with it, a change of the expression's form fails here"""
    src = open(os.path.join(CSRC, "new2all.hip")).read()
    hdr = open(os.path.join(CSRC, "engine_internal.h")).read()
    assert _LDS_TEXT in src, "new2all.hip no longer holds `%s`: restate new2all_cases.lds_limits" % _LDS_TEXT
    assert re.search(r"constexpr uint32_t KMDB_CK_IDS = %d;" % CK_IDS, hdr) and re.search(r"const uint32_t qcap = %d;" % QCAP, src)
    assert "uint32_t threads = 512;" in src and "if (atoi(ev) == 1024) threads = 1024;" in src
    m = re.search(r"lds_hist = N \* (\d+) \+ qcap \* (\d+) \+ threads \* (\d+) \+ (\d+) <= (\d+) \* (\d+);", src)
    a, b, c, d, e, f = (int(x) for x in m.groups())
    return {t: (e * f - d - c * t - b * QCAP) // a for t in THREADS}


def key_bits(P, nq):
    """(pbits, qbits) of the sorted key (n2a_run): 2^pbits > patterns, 2^qbits >= queries"""
    pbits = qbits = 1
    while (1 << pbits) <= P:
        pbits += 1
    while (1 << qbits) < nq:
        qbits += 1
    return pbits, qbits


# ------------------------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------------------------
class Tables:
    """256 linear-probing tables of chosen capacities, filled slot by slot"""

    def __init__(self, caps):
        self.caps = np.asarray(caps, dtype=np.int64)
        assert self.caps.size == N_BUCKETS
        self.boff = np.zeros(N_BUCKETS + 1, dtype=np.uint64)
        self.boff[1:] = np.cumsum(self.caps).astype(np.uint64)
        self.slots = np.full(int(self.boff[-1]), EMPTY, dtype=np.uint64)
        self._next = 1

    def fresh(self, cap, home):
        """a 32-bit key that no call returned before whose home slot in a table of `cap` slots is `home`"""
        key = keys_with_home(cap, home, 1, self._next)[0]
        self._next = key + 1
        return key

    def put(self, b, slot, key, pid):
        i = int(self.boff[b]) + slot
        assert 0 <= slot < self.caps[b] and self.slots[i] == EMPTY and 0 <= pid < EMPTY_VAL
        self.slots[i] = np.uint64(key) | (np.uint64(pid) << np.uint64(32))
        return (b << 32) | key

    def place(self, b, slot, home, pid):
        """a fresh key of home slot `home` at `slot` of bucket b -> its word"""
        cap = int(self.caps[b])
        return self.put(b, slot % cap, self.fresh(cap, home % cap), pid)

    def absent(self, b, home):
        """a word of bucket b that is in no table, with home slot `home`"""
        cap = int(self.caps[b])
        return (b << 32) | self.fresh(cap, home % cap)

    def insert(self, word, pid):
        """linear probing from the home slot (the walk cases: where a key lands is not the point)"""
        b, key = word >> 32, word & 0xffffffff
        cap, off = int(self.caps[b]), int(self.boff[b])
        s = fmix32(key) & (cap - 1)
        while self.slots[off + s] != EMPTY:
            s = (s + 1) & (cap - 1)
        self.put(b, s, key, pid)

    def check(self):
        """every table is a valid hashmap_lp table"""
        vals = (self.slots >> np.uint64(32)).astype(np.int64)
        keys = (self.slots & np.uint64(0xffffffff)).astype(np.int64)
        for b in range(N_BUCKETS):
            cap, off = int(self.caps[b]), int(self.boff[b])
            assert cap >= 1 and cap & (cap - 1) == 0, (b, cap)
            used = vals[off: off + cap] != EMPTY_VAL
            assert not used.all(), "bucket %d has no empty slot" % b
            assert (keys[off: off + cap][~used] == 0).all()
            mine = keys[off: off + cap][used]
            assert np.unique(mine).size == mine.size, "bucket %d holds a key twice" % b
            for s in np.nonzero(used)[0].tolist():
                h = fmix32(int(keys[off + s])) & (cap - 1)
                while h != s:
                    assert used[h], "bucket %d: the key at slot %d is cut off from its home by the empty slot %d" % (b, s, h)
                    h = (h + 1) & (cap - 1)
        return self

    def dictionary(self):
        """(sorted words, pattern of each), read back from the slots"""
        bucket = np.repeat(np.arange(N_BUCKETS, dtype=np.uint64), self.caps)
        used = (self.slots >> np.uint64(32)) != np.uint64(EMPTY_VAL)
        words = (bucket[used] << np.uint64(32)) | (self.slots[used] & np.uint64(0xffffffff))
        order = np.argsort(words)
        return words[order], (self.slots[used] >> np.uint64(32)).astype(np.int64)[order]


def probe_census(T, word):
    """kmdb_probe (csrc/hash_probe.h) restated for one word: which path, what it walks and where it ends.  path: "none" (bucket beyond
    the tables), "scalar" (cap < 4 or an odd offset) or "four"; steps: slots a linear probe compares; end: the slot that ended it; wrapped:
    it went from the last slot to slot 0; groups: the four-slot loads of the "four" path; skipped_empty: an EMPTY slot of the home group
    lies before `first`; round5: the load that ended the probe was the revisit of the home group (seen == cap)."""
    b, key = word >> 32, word & 0xffffffff
    if b >= N_BUCKETS:
        return {"path": "none", "found": False, "pid": None}
    cap, off = int(T.caps[b]), int(T.boff[b])
    tab = T.slots[off: off + cap]
    val = lambda s: int(tab[s] >> np.uint64(32))        # noqa: E731
    home = fmix32(key) & (cap - 1)
    s, steps, wrapped = home, 0, False
    while True:
        steps += 1
        assert steps <= cap
        if val(s) == EMPTY_VAL or int(tab[s] & np.uint64(0xffffffff)) == key:
            break
        wrapped |= s == cap - 1
        s = (s + 1) & (cap - 1)
    found = val(s) != EMPTY_VAL
    out = {"bucket": b, "cap": cap, "off": off, "home": home, "first": home & 3, "steps": steps, "end": s, "wrapped": wrapped,
           "found": found, "pid": val(s) if found else None, "path": "scalar" if cap < 4 or off & 1 else "four"}
    if out["path"] == "four":
        g, first, groups, got = home & ~3, home & 3, 0, None
        out["skipped_empty"] = any(val(g + t) == EMPTY_VAL for t in range(first))
        seen = 0
        while seen < cap + 4 and got is None:
            groups += 1
            for t in range(first, 4):
                if val(g + t) == EMPTY_VAL or int(tab[g + t] & np.uint64(0xffffffff)) == key:
                    got = g + t
                    break
            first, g, seen = 0, (g + 4) & (cap - 1), seen + 4
        assert got == s
        out["groups"], out["round5"] = groups, groups == cap // 4 + 1
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, N, pat, tables, queries, **about):
        import torch
        self.name, self.N, self.T, self.about = name, N, tables.check(), about
        self.kmers, self.pids = tables.dictionary()
        self.P = int(pat["parent"].numel())
        assert (self.pids >= 1).all() and (self.pids < self.P).all()
        self.pat = dict(pat)
        self.pat["num_kmers"] = torch.from_numpy(np.bincount(self.pids, minlength=self.P).astype(np.int64))
        self.queries = [np.unique(np.asarray(q, dtype=np.uint64)) for q in queries]
        self.path = None

    @functools.lru_cache(maxsize=None)
    def full(self):
        full = V.full_lists(self.pat)
        for f in full:
            assert f.size == 0 or ((np.diff(f) > 0).all() and f[-1] < self.N)
        return full

    def hits(self, q):
        """(hit patterns ascending, k-mers of the query under each): the words of q that the dictionary holds"""
        if not self.kmers.size or not q.size:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        at = np.minimum(np.searchsorted(self.kmers, q), self.kmers.size - 1)
        return np.unique(self.pids[at[self.kmers[at] == q]], return_counts=True)

    @functools.lru_cache(maxsize=None)
    def rows(self):
        """The rows from the definition (reference similarity_calculator.cpp:809-925): row[s] = the k-mers of the query that are in the
        dictionary and whose pattern's FULL list holds s.  No table, no tree walk."""
        full = self.full()
        out = np.zeros((len(self.queries), self.N), dtype=np.uint32)
        for qi, q in enumerate(self.queries):
            for p, c in zip(*(x.tolist() for x in self.hits(q))):
                out[qi, full[p]] += np.uint32(c)
        out.setflags(write=False)
        return out

    def write(self, S, path):
        """the case as a .db file in the reference's format, its fabricated tables included"""
        arr = S.to_view_arrays(self.pat)
        S.write_db(path, K_LEN, 1.0, ["s%d" % i for i in range(self.N)], [1] * self.N, arr, kmers_count=int(self.kmers.size),
                   tables=(self.T.boff, self.T.slots))
        self.path = path
        return path

    @functools.lru_cache(maxsize=None)
    def layout(self):
        """the forest in DFS order as the upload lays it out: (dfs index of a pattern, parent and local-list length by dfs index)"""
        d = dfs_index(self.pat)
        par, nloc = self.pat["parent"].numpy(), self.pat["num_local"].numpy()
        pd, ld, size = np.full(self.P, -1, dtype=np.int64), np.zeros(self.P, dtype=np.int64), np.ones(self.P, dtype=np.int64)
        for p in range(self.P - 1, -1, -1):
            ld[d[p]] = nloc[p]
            if par[p] >= 0:
                pd[d[p]] = d[par[p]]
                size[par[p]] += size[p]
        se = np.zeros(self.P, dtype=np.int64)
        se[d] = d + size
        return d, pd, ld, se

    @functools.lru_cache(maxsize=None)
    def walk_census(self, threads):
        """The walk's bookkeeping restated: the batch's sorted runs (query, DFS index of the hit pattern, k-mers), thread i of workgroup
        i // threads takes run i; node r is visited by hit i of a query iff r is an ancestor-or-self of h_i and r > h_(i-1).
        -> runs [(query, dfs, count)], visited [[nodes of run i]], per (workgroup, query): hits and long lists filed"""
        d, pd, ld, se = self.layout()
        runs, visited, groups = [], [], {}
        for qi, q in enumerate(self.queries):
            p, c = self.hits(q)
            order = np.argsort(d[p])
            prev = -1
            for h, n in zip(d[p][order].tolist(), c[order].tolist()):
                seen, r = [], h
                while r > prev:
                    seen.append(r)
                    r = int(pd[r])
                g = groups.setdefault((len(runs) // threads, qi), {"hits": 0, "queued": 0})
                g["hits"] += 1
                g["queued"] += sum(int(ld[x]) > CK_IDS for x in seen)
                runs.append((qi, h, n))
                visited.append(seen)
                prev = h
        return runs, visited, groups


def _pids(P):
    """patterns 1 .. P - 1 round and round"""
    n = 0
    while True:
        yield 1 + n % (P - 1)
        n += 1


def _tiny_forest():
    """N = 48, 41 patterns: 20 roots of two ids, a child under each"""
    F = V._Forest()
    for j in range(20):
        F.add([j, 24 + j % 7], -1, 0)
    for j in range(20):
        F.add([32 + (5 * j) % 16], 1 + j, 0)
    return F.pat(), 48


P1_CAPS = (1, 16, 1, 4, 2, 8, 2, 2, 16, 1, 4, 1, 16, 2, 1, 4)       # 81 slots: the next cycle starts at the other parity


def _rot(pl, r):
    return [(s + r, h + r) for s, h in pl]


def _probe_case(name, caps, recipe, extra=None):
    """tables of `caps`; recipe(b, cap) -> ([(slot, home)], [homes of absent keys]).  Queries: the words of every bucket, everything at
    once, and every word of the first 16 buckets alone."""
    pat, N = _tiny_forest()
    T = Tables(caps)
    pid = _pids(41)
    per_bucket, labels = [], {}
    for b in range(N_BUCKETS):
        placed, absent = recipe(b, int(T.caps[b]))
        words = [T.place(b, s, h, next(pid)) for s, h in placed]
        words += [T.absent(b, h) for h in absent]
        per_bucket.append(words)
    queries = [w for w in per_bucket]
    if extra:
        queries += extra(T, pid)
    everything = [w for q in queries for w in q]
    queries = queries + [everything] + [[w] for ws in per_bucket[:16] for w in ws]
    return Case(name, N, pat, T, queries, probes=sorted(set(everything)), labels=labels)


def _p1_recipe(b, cap):
    if cap == 1:
        return [], [0]
    if cap == 2:
        return [(b & 1, b & 1)], [b & 1, 1 - (b & 1)]
    if cap == 4:
        return _rot([(1, 1), (2, 1), (3, 3)], b // 3), [0, 1, 2, 3]
    if cap == 8:
        return _rot([(6, 6), (7, 6), (0, 7), (1, 0), (2, 6)], b // 5), list(range(8))
    return _rot([(13, 13), (14, 13), (15, 14), (0, 15), (1, 13), (2, 0), (5, 5), (6, 5), (7, 6), (8, 8), (10, 10)], b // 7), list(range(16))


def _p2_recipe(b, cap):
    r, G = (b // 3) % 8, cap // 2
    if cap == 4:
        if r < 4:
            return [(r, r)], [0, 1, 2, 3]
        return ([(2, 2), (3, 2), (0, 2)], [(3, 3), (0, 3), (1, 3)], [(1, 1), (2, 1), (3, 1)], [(1, 1)])[r - 4], ([2, 3, 0, 1], [3, 0, 1, 2], [1, 2, 3, 0], [1, 2])[r - 4]
    return ([(0, 0), (5, 5), (10, 10), (15, 15)], [(2, 2), (3, 2), (4, 2), (5, 2)], [(cap - 1, cap - 1), (0, cap - 1), (1, cap - 1)],
            [(G + 1, G + 1), (G + 2, G + 1), (G + 3, G + 1), (G + 4, G + 1)], [(5, 5)])[r % 5], \
           ([0, 5, 10, 15, 1], [2, 3, 4, 5], [cap - 1, 0, 1, 2], [G + 1, G + 2, G + 3, G + 4, G], [5, 6])[r % 5]


def _p3_recipe(b, cap):
    if cap == 4:                                        # e = 0: slots 1, 2, 3 full, the key stored at 3 has home 1
        return [(1, 1), (2, 1 + (b // 2) % 2), (3, 1)], [1, 2, 3, 0]
    e = 4 * ((b // 2) % 4)
    home = {e + 15: e + 1, e + 4: e + 1, e + 8: e + 2, e + 12: e + 3}
    return [(e + j, home.get(e + j, e + j)) for j in range(1, 16)], [e + 1, e + 2, e + 3, e]


def _p4_extra(T, pid):
    """buckets 1, 8, 17 (capacity 16) and 5 (capacity 8) are left empty by the recipe and filled here"""
    shared = T.fresh(16, 3)                             # one 32-bit key in three buckets, three patterns
    words = [T.put(1, 0, 0, 7),                         # key 0 at its home (fmix32(0) = 0)
             T.place(8, 0, 0, 9), T.put(8, 1, 0, 11),   # key 0 behind another key of home 0
             T.place(17, 1, 1, 13), T.place(17, 15, 15, 14)]          # bucket 17: key 0 absent, its home slot 0 empty between full slots
    words += [T.put(b, s, shared, p) for b, s, p in ((1, 3, 21), (8, 3, 22), (17, 3, 23))]
    words += [T.put(5, fmix32(shared) & 7, shared, 24)]
    zero = [(b << 32) | 0 for b in (1, 8, 17, 5, 0)]    # (bucket 0: capacity 1, empty)
    beyond = [(1 << 40) | words[0], (0xFFFFFF << 40) | (8 << 32)]          # bits above 2k: bucket >= 256
    return [words, zero, [zero[2]], [(3 << 32) | shared, (1 << 32) | shared], beyond, beyond + words[:2]]


def _p4_recipe(b, cap):
    if b in (1, 8, 17, 5):
        return [], []
    return _p1_recipe(b, cap)


def _caps_for(counts):
    """the smallest power of two above the number of keys of every bucket: tables of 1, 2, 4, ... slots, nearly full"""
    return [1 << int(c).bit_length() for c in counts]


def _walk_case(name, N, pat, rng, kmers_of, make_queries, **about):
    """kmers_of[p]: how many k-mers pattern p gets (random distinct 40-bit words, inserted by linear probing into tables just large enough)
    make_queries(words_of) -> the batch, words_of[p] the words of pattern p; rng.absent(n): words that are in no table"""
    P = int(pat["parent"].numel())
    total = int(sum(kmers_of))
    u = rng.permutation(np.unique(rng.integers(0, 1 << 40, size=total + total // 4 + 4096, dtype=np.int64)))
    assert u.size >= total + 2048
    own, spare = u[:total], u[total:]
    T = Tables(_caps_for(np.bincount(own >> 32, minlength=N_BUCKETS)))
    words_of, at = [[] for _ in range(P)], 0
    for p in range(P):
        words_of[p] = own[at: at + kmers_of[p]].tolist()
        at += kmers_of[p]
        for w in words_of[p]:
            T.insert(w, p)
    return Case(name, N, pat, T, make_queries(words_of, spare.tolist()), **about)


def case_w1():
    rng = np.random.default_rng(1801)
    N, F = 128, V._Forest()
    deep = {(c, l): [] for c in (1, 2, 3) for l in (33, 32)}
    plan = [(c, 33) for c, n in ((1, 660), (2, 520), (3, 490)) for _ in range(n)] + [(c, 32) for c in (1, 2, 3) for _ in range(10)]
    for i in rng.permutation(len(plan)).tolist():
        c, l = plan[i]
        par, w = -1, N // c
        for j in range(c):
            lo, hi = j * w, (N if j == c - 1 else (j + 1) * w)
            ids = (rng.choice(hi - lo, size=l, replace=False) + lo).tolist()
            if j == c - 1 and i % 4 == 0 and N - 1 not in ids:
                ids.remove(max(ids))
                ids.append(N - 1)
            par = F.add(ids, par, 0)
        deep[(c, l)].append(par)
    pat = F.pat()
    kmers_of = np.zeros(len(F.locs), dtype=np.int64)
    for v in deep.values():
        for i, p in enumerate(v):
            kmers_of[p] = 1 + i % 3
    mix = ((1, 511, 0), (1, 510, 1), (0, 511, 1), (0, 36, 476), (648, 276, 100))         # 1023, 1024, 1025, 1500 in 512 hits; 1500 in 1024

    def queries(words_of, spare):
        qs = []
        for qi, (a, b, c) in enumerate(mix):
            pats = [p for k, n in ((1, a), (2, b), (3, c)) for p in deep[(k, 33)][qi: qi + n]]
            qs.append([w for p in pats for w in words_of[p]] + spare[qi * 10: qi * 10 + 7])
        twins = [p for k in (1, 2, 3) for p in deep[(k, 32)]]
        qs.append([w for p in twins for w in words_of[p]])
        qs.append([w for p in twins[::2] + deep[(3, 33)][:40] + deep[(1, 33)][:5] for w in words_of[p]])
        return qs
    return _walk_case("W1", N, pat, rng, kmers_of.tolist(), queries, mix=mix, targets=(1023, 1024, 1025, 1500, 1500))


def case_w2():
    rng = np.random.default_rng(1802)
    N, F = 200, V._Forest()
    leaf = lambda par, i: F.add(rng.choice(np.arange(4, N), size=(36 if i % 150 == 7 else 1 + i % 3), replace=False), par, 0)      # noqa: E731
    before = [F.add([int(rng.integers(0, N))], -1, 0) for _ in range(20)]
    R = F.add([0, 1], -1, 0)
    A = F.add([2], R, 0)
    under = [A] + [leaf(A, i) for i in range(600)]
    fam = []
    for n_kids in (421, 511, 480):                      # the family nodes are hits 601, 1023 and 1535 of the subtree
        f = F.add([3], R, 0)
        fam.append(f)
        under += [f] + [leaf(f, i) for i in range(n_kids)]
    after = [F.add([int(rng.integers(0, N))], -1, 0) for _ in range(20)]
    pat = F.pat()
    P = len(F.locs)
    kmers_of = np.array([0 if p in (0, R) else (300 if p % 97 == 5 else 1 + p % 4) for p in range(P)], dtype=np.int64)
    pool = before + under + after                       # pattern-id order == DFS order here
    picks = ((3, 0, 511), (2, 1, 512), (3, 1, 513), (1, 10, 1024), (1, 0, 1025))

    def queries(words_of, spare):
        qs = [[w for p in under for w in words_of[p]]]
        for qi, (step, first, n) in enumerate(picks):
            pats = pool[first::step][:n]
            assert len(pats) == n
            qs.append([w for p in pats for w in words_of[p][: 1 + (p + qi) % len(words_of[p])]] + spare[qi * 20: qi * 20 + 11])
        return qs
    return _walk_case("W2", N, pat, rng, kmers_of.tolist(), queries, R=R, A=A, fam=fam, under=len(under), picks=picks)


def _w3(name, P):
    from test_gpu_parity import _random_forest
    rng = np.random.default_rng(1803 + P)
    N = 96
    pat = _random_forest(rng, N, P, 3, chain_frac=0.3)
    d = dfs_index(pat)
    last = int(np.nonzero(d == P - 1)[0][0])
    kmers_of = [0] + [1 + p % 2 for p in range(1, P)]

    def queries(words_of, spare):
        single = [[words_of[1 + (7 * i) % (P - 1)][0]] for i in range(599)]
        rep = [w for p in range(3, P, 25) for w in words_of[p]] + spare[:5]
        miss = lambda j: spare[100 + 9 * j: 100 + 9 * j + 1 + 4 * j]          # noqa: E731
        qs = [[], miss(0)] + single[:198] + [[], miss(1)] + single[198:296] + [rep, rep] + single[296:394] + [miss(2), []] + \
            single[394:440] + [rep] + single[440:488] + [[], miss(3)] + single[488:] + [miss(4), [], [words_of[last][0]]]
        return qs
    c = _walk_case(name, N, pat, rng, kmers_of, queries, last=last)
    assert len(c.queries) == 613
    return c


def _w4(N):
    from test_gpu_parity import _random_forest
    rng = np.random.default_rng(1804)                   # (one forest plan for the four sizes)
    F = forest_of(_random_forest(rng, N, 2500, 40, chain_frac=0.3))
    edge = []
    for lo, n in ((100, 3000), (2500, 700), (5000, 4000), (N - 2100, 2000)):           # clades: runs of consecutive ids, a child, a grandchild
        c = F.add(range(lo, lo + n), -1, 0)
        g = F.add(range(lo + n, lo + n + 40), c, 0)
        edge += [c, g, F.add([lo + n + 50, N - 1], g, 0)]
    for last in (N - 1, N - 2):                         # queued lists whose last run ends at N - 1 / N - 2: one run, and many
        edge.append(F.add(range(last - 49, last + 1), -1, 0))
        edge.append(F.add(list(range(last - 120, last - 40, 2)) + [last - 1, last], -1, 0))
        edge.append(F.add(list(range(20, 100, 2)) + [last], -1, 0))
    pat = F.pat()
    P = len(F.locs)
    kmers_of = (rng.integers(0, 3, size=P)).tolist()
    kmers_of[0] = 0
    for p in edge:
        kmers_of[p] = 2

    def queries(words_of, spare):
        have = [p for p in range(P) if words_of[p]]
        qs = []
        for qi in range(5):
            pats = rng.choice(have, size=300, replace=False).tolist() + edge[qi::2]
            qs.append([w for p in pats for w in words_of[p][: 1 + qi % 2]] + spare[qi * 50: qi * 50 + 40])
        qs.append([w for p in edge for w in words_of[p]])
        return qs
    return _walk_case("W4_%d" % N, N, pat, rng, kmers_of, queries, edge=edge)


def case_w5():
    rng = np.random.default_rng(1805)
    N, F = 131200, V._Forest()
    roots, kids, grand = [], [], []
    for n, first, tail in ((65534, 0, (131100, 131102, 131150)), (65535, 1, (131101, 131105, 131199)), (65536, 0, (131072, 131080, 131198))):
        r = F.add(np.arange(n) * 2 + first, -1, 0)
        c = F.add(tail[:2], r, 0)
        roots.append(r); kids.append(c); grand.append(F.add([tail[2]], c, 0))
    r = F.add(np.arange(100, 70100), -1, 0)
    c = F.add([70100, 70102], r, 0)
    roots.append(r); kids.append(c); grand.append(F.add([131000, N - 1], c, 0))
    pat = F.pat()
    kmers_of = [0] * len(F.locs)
    for i, (c, g) in enumerate(zip(kids, grand)):
        kmers_of[c], kmers_of[g] = 1, 2 + i

    def queries(words_of, spare):
        qs = [words_of[g] + spare[i: i + 2] for i, g in enumerate(grand)]
        return qs + [[w for g in grand for w in words_of[g]], [w for c in kids for w in words_of[c]] + words_of[grand[0]][:1]]
    return _walk_case("W5", N, pat, rng, kmers_of, queries, roots=roots, kids=kids, grand=grand)


BUILDERS = {
    "P1": lambda: _probe_case("P1", P1_CAPS * 16, _p1_recipe),
    "P2": lambda: _probe_case("P2", ((4, 16, 64) * 86)[:N_BUCKETS], _p2_recipe),
    "P3": lambda: _probe_case("P3", (16, 4) * 128, _p3_recipe),
    "P4": lambda: _probe_case("P4", P1_CAPS * 16, _p4_recipe, _p4_extra),
    "W1": case_w1, "W2": case_w2,
    "W3a": lambda: _w3("W3a", 1023), "W3b": lambda: _w3("W3b", 1024),
    "W4_11008": lambda: _w4(11008), "W4_11009": lambda: _w4(11009), "W4_9984": lambda: _w4(9984), "W4_9985": lambda: _w4(9985),
    "W5": case_w5,
}
NAMES = tuple(BUILDERS)
PROBE = ("P1", "P2", "P3", "P4")
LARGE = ("W4_11008", "W4_11009", "W4_9984", "W4_9985", "W5")


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def in_range(c, q):
    """the words of a query whose bucket the tables have (the reference's reader is not handed the others)"""
    return q[(q >> np.uint64(32)) < np.uint64(N_BUCKETS)]


def probes_part(c, n_samples=32):
    """group P's second part for db2db: the probed words of the case (those of a bucket the tables have) as the k-mers of n_samples
    samples, word i in sample i % n_samples alone -> (forest, N, sorted words, pattern of each)"""
    F = V._Forest()
    for s in range(n_samples):
        F.add([s], -1, 0)
    words = in_range(c, np.array(c.about["probes"], dtype=np.uint64))
    return F.pat(), n_samples, words, 1 + np.arange(words.size, dtype=np.int64) % n_samples
