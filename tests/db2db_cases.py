"""Inputs and references of test_db2db_conformance.py: pairs of pattern forests with FABRICATED dictionaries (db2db looks k-mers up, it
never extracts them) that fix, for chosen (row pattern, column pattern) pairs, exactly how many k-mers the two share — by putting the
same k-mers into both dictionaries under those patterns — the definition of the cell in numpy, and a census that proves on the host
what the cases hold.  Host only.

A part is a forest in the format of synth.build_patterns (see variant_cases.py) plus its dictionary (sorted k-mers, the pattern of each);
num_kmers is the bincount of the k-mers' patterns.  A case is a row part, a column part and the pairs it planned; what the pairs ARE is
read back from the two dictionaries (np.intersect1d), never taken from the plan.

The engine's thresholds the cases are built around are restated in geometry() / first_pool_slots() with the lines of csrc/db2db.hip
they restate; engine_constants() reads the constants and checks the formulas' text in the source, so that a later change of a formula
fails the census (test_cases_hold_what_the_gpu_tests_rely_on) and not the reader.

Cases (test_db2db_conformance.py's docstring says which branch of the engine each one is for):
  S   4096 x 4096 samples (list store, 64 x 64 blocks: radix sort), heavy pairs with counts either side of 2^dbits, dbits = 17
  C   8255 x 4159 samples (root-path climb, 129 x 65 blocks, partial last blocks), heavy pairs either side of 2^16
  K1  pattern counts 512 x 511, K2: 2 x 256; the last DFS nodes of both sides and (first, last) share k-mers
  E2047 / E2048 / E2050   23 x 89, 32 x 64, 41 x 50 blocks: either side of the one-pass counting sort's limit
  P   tens of patterns whose full lists cover every block of C's geometry: more block records than the first pool holds; Ps: its
      scaled-down copy (520 x 260 samples) for the CPU oracle
  Z0  disjoint dictionaries; Z1: a column part of one sample; Z2: 65 samples x 1 sample; Zself: a part of 300 samples against itself"""
import functools
import os
import re

import numpy as np

import variant_cases as V

K_LEN = 18
ROOT = V.ROOT
CSRC = os.path.join(ROOT, "kmer-db_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------------------------------
# the engine's geometry, restated
# ------------------------------------------------------------------------------------------------------------------------------------
def geometry(nr, nc):
    """csrc/db2db.hip:447 (blocks of 64 ids) and :499-501: 2^key_bits > block pairs + 1 (a never-written slot's all-ones key lies beyond
    the streams), the digit width of a count is what 32 bits leave beside the key and the two bits of the digit's index"""
    nbr, nbc = (nr + 63) // 64, (nc + 63) // 64
    n_states = nbr * nbc
    key_bits = 1
    while (1 << key_bits) <= n_states + 1:
        key_bits += 1
    return {"nbr": nbr, "nbc": nbc, "n_states": n_states, "key_bits": key_bits, "dbits": 32 - key_bits - 2}


def digits(c, dbits):
    """the base-2^dbits digits of a count, lowest first (d2_emit_kernel, db2db.hip:246-248, 264-265)"""
    out = []
    while c:
        out.append(c & ((1 << dbits) - 1))
        c >>= dbits
    return out


def first_pool_slots(npairs, nr, nc):
    """slots of the record pool's FIRST attempt (db2db.hip:503-506: waves per workgroup and grid; :529, 547-549: six records per pair, an
    eighth for the grab tails, the waves' share and a floor of 130 grabs per cursor)"""
    k = engine_constants()
    g = geometry(nr, nc)
    wave_lds = (2 * (g["nbr"] + g["nbc"]) + ((g["nbr"] + g["nbc"]) * 2 + 7) // 8) * 8           # d2_wave_words, :186
    wpb = max(1, min(4, (150 << 10) // wave_lds))
    grid = min((npairs + wpb - 1) // wpb, 256 * 8)
    total = 6 * npairs
    grabs = (total + total // 8) // k["D2_GRAB"] // k["D2_CURSORS"] + grid * wpb // k["D2_CURSORS"] + 130
    return grabs * k["D2_GRAB"] * k["D2_CURSORS"]


# the formulas above as the source has them: engine_constants() fails when one of them is no longer there
_DB2DB_TEXT = ("while ((1ull << key_bits) <= (uint64_t)nbr * nbc + 1) ++key_bits;",
               "const uint32_t dbits = (uint32_t)(32 - key_bits - 2);",
               "unsigned long long total = 6ull * nruns;",
               "const uint64_t grabs = (total + total / 8) / D2_GRAB / D2_CURSORS + (uint64_t)grid * wpb / D2_CURSORS + 130;",
               "const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)nruns + wpb - 1) / wpb, 256 * 8);",
               "while ((1ull << cbits) <= ec.P) ++cbits;", "while ((1ull << rbits) <= er.P) ++rbits;")
_A2A_TEXT = ("if (n_states <= CS_MAX_KEYS) {", "inline uint32_t wide_digit_bits(int key_bits) { return (uint32_t)(32 - key_bits - 2); }")


@functools.lru_cache(maxsize=None)
def engine_constants():
    """CS_MAX_KEYS (a2a_blocks.hip:2222, the branch of kmdb_rect_sort_apply at :3191), D2_GRAB / D2_CURSORS (db2db.hip:184) and
    D2_SETS_MAX_NB (:132: the list store's limit in blocks), read from the source"""
    d2 = open(os.path.join(CSRC, "db2db.hip")).read()
    a2a = open(os.path.join(CSRC, "a2a_blocks.hip")).read()
    for text, src, name in [(t, d2, "db2db.hip") for t in _DB2DB_TEXT] + [(t, a2a, "a2a_blocks.hip") for t in _A2A_TEXT]:
        assert text in src, "%s no longer holds `%s`: restate db2db_cases.geometry / first_pool_slots" % (name, text)
    out = {}
    for name, src in (("CS_MAX_KEYS", a2a), ("D2_GRAB", d2), ("D2_CURSORS", d2), ("D2_SETS_MAX_NB", d2)):
        m = re.search(r"constexpr uint32_t [^;]*\b%s = (\d+)" % name, src)
        assert m, name
        out[name] = int(m.group(1))
    return out


def key_widths(P_row, P_col):
    """(rbits, cbits) of the pattern-pair key (db2db.hip:469-471): 2^bits > patterns of the part"""
    b = lambda P: max(1, int(P).bit_length())           # noqa: E731
    return b(P_row), b(P_col)


# ------------------------------------------------------------------------------------------------------------------------------------
# forests
# ------------------------------------------------------------------------------------------------------------------------------------
def _random_forest(*a, **kw):
    from test_gpu_parity import _random_forest as f
    return f(*a, **kw)


def forest_of(pat, remap=None):
    """a variant_cases._Forest holding the patterns of a forest dict (so that patterns can be added); remap: new id of every id, ascending"""
    lp, ids, par = pat["local_ptr"].numpy(), pat["local_ids"].numpy(), pat["parent"].numpy()
    F = V._Forest()
    for p in range(1, par.size):
        loc = ids[lp[p]: lp[p + 1]]
        F.add(loc if remap is None else remap[loc], int(par[p]), 0)
    return F


def dfs_index(pat):
    """pattern id -> DFS index as the upload lays the forest out (csrc/layout.hip:6-10: pre-order, the roots and the children of a node
    in pattern-id order).  The engine's pair key is made of these, not of pattern ids."""
    par = pat["parent"].numpy()
    P = par.size
    kids = [[] for _ in range(P + 1)]                   # kids[P]: the roots
    for p in range(P):
        kids[par[p] if par[p] >= 0 else P].append(p)
    out, n, stack = np.zeros(P, dtype=np.int64), 0, list(reversed(kids[P]))
    while stack:
        p = stack.pop()
        out[p] = n
        n += 1
        stack.extend(reversed(kids[p]))
    assert n == P
    return out


def n_blocks_of(full):
    return int(np.unique(full // 64).size)


# ------------------------------------------------------------------------------------------------------------------------------------
# parts and cases
# ------------------------------------------------------------------------------------------------------------------------------------
class Part:
    def __init__(self, pat, N, kmers, pids):
        import torch
        order = np.argsort(kmers)
        self.N, self.kmers, self.pids = N, kmers[order], pids[order].astype(np.int64)
        self.P = int(pat["parent"].numel())
        assert np.unique(self.kmers).size == self.kmers.size and (self.pids >= 1).all() and (self.pids < self.P).all()
        self.pat = dict(pat)
        self.pat["num_kmers"] = torch.from_numpy(np.bincount(self.pids, minlength=self.P).astype(np.int64))
        self.path = None

    @functools.lru_cache(maxsize=None)
    def full(self):
        """the FULL sample list of every pattern: its local ids behind its parent's list"""
        full = V.full_lists(self.pat)
        for f in full:
            assert f.size == 0 or ((np.diff(f) > 0).all() and f[-1] < self.N)
        return full

    def write(self, S, path):
        """the part as a .db file in the reference's format, hashtables included"""
        import torch
        arr = S.to_view_arrays(self.pat)
        tables = S.build_hashtables(torch.from_numpy(self.kmers.astype(np.int64)), torch.from_numpy(self.pids), K_LEN)
        S.write_db(path, K_LEN, 1.0, ["s%d" % i for i in range(self.N)], [1] * self.N, arr, kmers_count=int(self.kmers.size), tables=tables)
        self.path = path
        return path


class Case:
    """row part, column part (the same object: a part against itself), the pairs that were planned and what the case is about"""

    def __init__(self, name, row, col, planned, **about):
        self.name, self.row, self.col, self.planned, self.about = name, row, col, planned, about
        self.geo = geometry(row.N, col.N)

    @functools.lru_cache(maxsize=None)
    def pairs(self):
        """(row pattern, column pattern, shared k-mers) of every pair that shares k-mers, read from the two dictionaries"""
        _, ia, ib = np.intersect1d(self.row.kmers, self.col.kmers, assume_unique=True, return_indices=True)
        key, c = np.unique(self.row.pids[ia] * self.col.P + self.col.pids[ib], return_counts=True)
        return key // self.col.P, key % self.col.P, c.astype(np.int64)

    @functools.lru_cache(maxsize=None)
    def definition(self):
        """The cell from the definition (reference similarity_calculator.cpp:1340-1500: every pair of patterns adds its count to every pair
        of samples of the two FULL lists): R^T . C . Cc with C[pr, pc] the shared k-mers and R, Cc the 0/1 matrices of the full lists, in
        integer arithmetic mod 2^32 — written out over the non-zeros of C and R (dense_product() is the same with matrices)."""
        pr, pc, c = self.pairs()
        full_r, full_c = self.row.full(), self.col.full()
        T = np.zeros((self.row.P, self.col.N), dtype=np.uint64)              # C . Cc
        for a, b, n in zip(pr.tolist(), pc.tolist(), c.tolist()):
            T[a, full_c[b]] += np.uint64(n)
        T = (T & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        out = np.zeros((self.row.N, self.col.N), dtype=np.uint32)            # R^T . (C . Cc); uint32 sums wrap: mod 2^32
        for a in np.unique(pr).tolist():
            out[full_r[a]] += T[a]
        out.setflags(write=False)
        return out

    def dense_product(self):
        """R^T . C . Cc with dense uint64 matrices (small cases only)"""
        pr, pc, c = self.pairs()
        Cm = np.zeros((self.row.P, self.col.P), dtype=np.uint64)
        Cm[pr, pc] = c.astype(np.uint64)
        R = np.zeros((self.row.P, self.row.N), dtype=np.uint64)
        Cc = np.zeros((self.col.P, self.col.N), dtype=np.uint64)
        for M, part in ((R, self.row), (Cc, self.col)):
            for p, f in enumerate(part.full()):
                M[p, f] = 1
        return ((R.T @ Cm @ Cc) & np.uint64(0xFFFFFFFF)).astype(np.uint32)

    @functools.lru_cache(maxsize=None)
    def census(self):
        """records: the block records of the cell, na . nb . nd per pair (non-empty blocks of both lists, digits of the count); streams:
        the block pairs that receive one; oracle_cost: the cell additions of the CPU oracle, |row list| . |column list| per k-mer"""
        pr, pc, c = self.pairs()
        full_r, full_c = self.row.full(), self.col.full()
        blk_r = {a: np.unique(full_r[a] // 64) for a in np.unique(pr).tolist()}
        blk_c = {b: np.unique(full_c[b] // 64) for b in np.unique(pc).tolist()}
        hit = np.zeros((self.geo["nbr"], self.geo["nbc"]), dtype=bool)
        records = cost = 0
        for a, b, n in zip(pr.tolist(), pc.tolist(), c.tolist()):
            records += blk_r[a].size * blk_c[b].size * len(digits(n, self.geo["dbits"]))
            cost += n * full_r[a].size * full_c[b].size
            hit[np.ix_(blk_r[a], blk_c[b])] = True
        return {"records": records, "streams": hit, "oracle_cost": cost, "n_pairs": int(pr.size), "largest": int(c.max()) if c.size else 0}


def _universe(rng, n):
    """n distinct 36-bit k-mers in random order"""
    u = np.unique(rng.integers(0, 1 << 36, size=n + n // 8 + 64, dtype=np.int64).astype(np.uint64))
    assert u.size >= n
    return rng.permutation(u)[:n]


def make_parts(rng, pat_r, Nr, pat_c, Nc, pairs, private=(150, 150)):
    """two parts whose dictionaries share exactly c k-mers under (pr, pc) for every (pr, pc, c) of pairs, and `private` k-mers each that
    the other does not hold (lookups that miss), spread over the patterns"""
    assert len({(a, b) for a, b, _ in pairs}) == len(pairs)
    prs, pcs, cs = (np.array([p[i] for p in pairs], dtype=np.int64) for i in range(3))
    total = int(cs.sum())
    u = _universe(rng, total + private[0] + private[1])
    Pr, Pc = int(pat_r["parent"].numel()), int(pat_c["parent"].numel())
    own_r, own_c = u[total: total + private[0]], u[total + private[0]:]
    row = Part(pat_r, Nr, np.concatenate([u[:total], own_r]), np.concatenate([np.repeat(prs, cs), rng.integers(1, Pr, size=own_r.size)]))
    col = Part(pat_c, Nc, np.concatenate([u[:total], own_c]), np.concatenate([np.repeat(pcs, cs), rng.integers(1, Pc, size=own_c.size)]))
    return row, col


def light_pairs(rng, rows, cols, n, taken=(), lo=1, hi=5):
    """n distinct pairs (row pattern of rows, column pattern of cols) that are not in `taken`, each sharing lo .. hi k-mers"""
    rows, cols = np.asarray(rows), np.asarray(cols)
    seen, out = set(taken), []
    if n == rows.size * cols.size and not seen:         # every pair
        cand = [(int(a), int(b)) for a in rows for b in cols]
    else:                                               # drawn at random: few enough that a draw is rarely a repeat
        assert n <= (rows.size * cols.size - len(seen)) // 2
        cand = []
        while len(cand) < n:
            p = (int(rows[rng.integers(rows.size)]), int(cols[rng.integers(cols.size)]))
            if p not in seen:
                seen.add(p)
                cand.append(p)
    for a, b in cand:
        out.append((a, b, int(rng.integers(lo, hi + 1))))
    return out


def heavy_counts(dbits):
    """counts either side of the digit boundary: 2^dbits - 1 (the largest of one digit), 2^dbits (low digit ZERO: a weight-0 record),
    2^dbits + 1, 2^(dbits + 1) - 1 (high digit 1, low digit all ones) and 3 . 2^dbits + 5"""
    b = 1 << dbits
    return [b - 1, b, b + 1, 2 * b - 1, 3 * b + 5]


def _heavy_case(name, seed, Nr, Nc, light_r, light_c, heavy_r, heavy_c, counts, n_light, desc):
    """S and C.  light_*: (patterns, longest local list) of the random forest; heavy_*: [(ids, parent)] — parent None: a root, "light": a
    child of a light ROOT; desc: (i, ids) — a light pattern of these ids under heavy_r[i].  The heavy pairs are (heavy_r[i], heavy_c[i]) with
    counts[i]; beyond len(heavy_r), the row pattern is heavy_r[0] and the column pattern heavy_c[1] (a row list serves two heavy pairs)."""
    rng = np.random.default_rng(seed)
    Fr = forest_of(_random_forest(rng, Nr, light_r[0], light_r[1], chain_frac=0.3))
    Fc = forest_of(_random_forest(rng, Nc, light_c[0], light_c[1], chain_frac=0.3))
    n_light_r, n_light_c = len(Fr.locs), len(Fc.locs)

    def add_heavy(F, spec, n_l):
        ids = []
        for loc, parent in spec:
            par = -1
            if parent == "light":                       # under a light root whose ids all lie before the heavy one's
                par = next(p for p in range(1, n_l) if F.parent[p] < 0 and F.locs[p][-1] < loc[0] and F.locs[p].size <= 2)
            ids.append(F.add(loc, par, 0))
        return ids
    hr, hc = add_heavy(Fr, heavy_r, n_light_r), add_heavy(Fc, heavy_c, n_light_c)
    desc = Fr.add(desc[1], hr[desc[0]], 0)              # a light pattern below a heavy one: it inherits its ids
    pat_r, pat_c = Fr.pat(), Fc.pat()
    heavy = []
    for i, c in enumerate(counts):
        heavy.append((hr[i], hc[i], c) if i < len(hr) else (hr[0], hc[1], c))
    pairs = list(heavy)
    taken = {(a, b) for a, b, _ in pairs}
    # light pairs of the descendant and of heavy patterns (a wave's pairs then change between one and two digits under one cached row list)
    extra = [(desc, 1 + i, 1 + i % 5) for i in range(0, 40, 3)] + [(hr[0], 2 + i, 1 + i % 3) for i in range(0, 30, 7)] + [(3 + i, hc[0], 2 + i % 4) for i in range(0, 30, 7)]
    pairs += extra
    taken |= {(a, b) for a, b, _ in extra}
    pairs += light_pairs(rng, range(1, n_light_r), range(1, n_light_c), n_light, taken)
    row, col = make_parts(rng, pat_r, Nr, pat_c, Nc, pairs)
    return Case(name, row, col, pairs, heavy=heavy, descendant=desc, heavy_rows=hr, heavy_cols=hc)


def case_s():
    """4096 x 4096: both parts at the list store's limit.  Heavy lists of 2 .. 4 ids: across the blocks 0 | 1, inside the last block (63: a
    full one) up to the last sample id, over four blocks, first and last block; one heavy column pattern hangs under a light root"""
    d = geometry(4096, 4096)["dbits"]
    return _heavy_case("S", 1701, 4096, 4096, (400, 12), (380, 12),
                       [([62, 66, 70], None), ([4040, 4095], None), ([1000, 2047, 2048, 3000], None), ([5, 4095], None)],
                       [([63, 64], None), ([4033, 4094, 4095], None), ([3900, 4000], "light"), ([2100, 2101], None)],
                       [heavy_counts(d)[i] for i in (0, 1, 2, 4, 3)], 1200, (0, [300, 1000, 4000]))


def case_c():
    """8255 x 4159: both parts beyond the store, both with a partial last block (block 128: 63 ids, block 64: 63 ids).  Heavy lists that
    end with the LAST sample id of their part on both sides"""
    d = geometry(8255, 4159)["dbits"]
    b = 1 << d
    return _heavy_case("C", 1702, 8255, 4159, (500, 15), (300, 12),
                       [([8190, 8254], None), ([100, 4000, 8000], None), ([4095, 4096], None), ([64, 8254], None)],
                       [([4096, 4158], None), ([0, 63, 64], None), ([3000, 3001], "light"), ([1, 4157], None)],
                       [b - 1, b, b + 1, 2 * b + 3], 1500, (2, [4200, 6000, 8200]))


def _key_case(name, seed, Nr, Pr, Nc, Pc, n_light):
    """pattern counts at 2^n / 2^n - 1: the pair key's widths change there, and the last DFS node's index is all ones but for the bit that
    keeps it apart from the "no hit" key.  (last, last), (first, last), (last, first) and (first, first) by DFS position share k-mers."""
    rng = np.random.default_rng(seed)

    def forest(N, P):
        if P == 2:
            F = V._Forest()
            F.add([3, 64, N - 1], -1, 0)
            return F.pat()
        return _random_forest(rng, N, P, 4, chain_frac=0.2)
    pat_r, pat_c = forest(Nr, Pr), forest(Nc, Pc)
    ends = []
    for pat in (pat_r, pat_c):
        d = dfs_index(pat)
        ends.append((int(np.nonzero(d == 1)[0][0]), int(np.nonzero(d == d.size - 1)[0][0])))
    (fr, lr), (fc, lc) = ends
    ends_c = {}
    for a, b, c in ((lr, lc, 3), (fr, lc, 2), (lr, fc, 4), (fr, fc, 1)):          # (with two patterns, first == last)
        ends_c.setdefault((a, b), c)
    pairs = [(a, b, c) for (a, b), c in ends_c.items()]
    pairs += light_pairs(rng, range(1, Pr), range(1, Pc), n_light, {(a, b) for a, b, _ in pairs})
    row, col = make_parts(rng, pat_r, Nr, pat_c, Nc, pairs)
    return Case(name, row, col, pairs, ends=ends)


def _block_space(N, kept):
    """the ids of the kept blocks of a part of N samples, ascending"""
    return np.concatenate([np.arange(b * 64, min((b + 1) * 64, N)) for b in kept])


def _sort_case(name, seed, nbr, nbc, full):
    """nbr x nbc blocks, both parts with a partial last block, light counts only.  full: two patterns on either side whose lists hold an
    id of EVERY block, paired: every block pair gets a record.  Otherwise the forests live in about half of the blocks of either part
    (the last block of the rows and the first of the columns among the empty ones): whole block rows and columns receive nothing."""
    rng = np.random.default_rng(seed)
    Nr, Nc = nbr * 64 - 3, nbc * 64 - 7
    pats, covers, kept = [], [], []
    for N, nb, drop in ((Nr, nbr, nbr - 1), (Nc, nbc, 0)):
        if full:
            F = forest_of(_random_forest(rng, N, 250, 8, chain_frac=0.2))
            cov = []
            for _ in range(2):
                cov.append(F.add([b * 64 + int(rng.integers(0, min(64, N - b * 64))) for b in range(nb)], -1, 0))
            kept.append(np.arange(nb))
        else:
            blocks = np.sort(rng.choice(np.setdiff1d(np.arange(nb), [drop]), size=nb // 2, replace=False))
            space = _block_space(N, blocks)
            F = forest_of(_random_forest(rng, space.size, 250, 8, chain_frac=0.2), remap=space)
            cov = []
            kept.append(blocks)
        pats.append(F.pat())
        covers.append(cov)
    pairs = [(a, b, 1 + (a + b) % 3) for a in covers[0] for b in covers[1]]
    pairs += light_pairs(rng, range(1, 250), range(1, 250), 800, {(a, b) for a, b, _ in pairs})
    row, col = make_parts(rng, pats[0], Nr, pats[1], Nc, pairs)
    return Case(name, row, col, pairs, full=full, kept=kept)


def _pool_case(name, seed, Nr, Nc):
    """Few patterns whose FULL lists hold an id of every block of their part — roots with one id per block (two in every seventh), 40 of
    the rows and 30 of the columns, and 20 children, four under each of 5 roots that cover the first half of the blocks, which cover
    the other half — 60 row and 50 column patterns, and every one of the 3000 pairs shares 1 .. 3 k-mers: 3000 . nbr . nbc block records."""
    rng = np.random.default_rng(seed)
    pats, paired = [], []
    for N, n_roots in ((Nr, 40), (Nc, 30)):
        nb = (N + 63) // 64
        ids_in = lambda blocks: sorted({b * 64 + int(rng.integers(0, min(64, N - b * 64))) for b in blocks for _ in range(2 if b % 7 == 3 else 1)})      # noqa: E731
        F = V._Forest()
        mine = [F.add(ids_in(range(nb)), -1, 0) for _ in range(n_roots)]
        for _ in range(5):
            half = F.add(ids_in(range(nb // 2)), -1, 0)
            mine += [F.add(ids_in(range(nb // 2, nb)), half, 0) for _ in range(4)]
        pats.append(F.pat())
        paired.append(mine)
    pairs = light_pairs(rng, paired[0], paired[1], len(paired[0]) * len(paired[1]), lo=1, hi=3)
    row, col = make_parts(rng, pats[0], Nr, pats[1], Nc, pairs)
    return Case(name, row, col, pairs, paired=paired)


def _one_sample_part():
    F = V._Forest()
    F.add([0], -1, 0)
    return F.pat()


def _degenerate_case(name):
    rng = np.random.default_rng({"Z0": 1730, "Z1": 1731, "Z2": 1732, "Zself": 1733}[name])
    if name == "Z0":                                    # nothing shared: no pair, no record, the cell stays zero
        row, col = make_parts(rng, _random_forest(rng, 100, 40, 6), 100, _random_forest(rng, 70, 30, 6), 70, [], private=(300, 300))
        return Case(name, row, col, [])
    if name in ("Z1", "Z2"):                            # a column part of ONE sample; Z2: 65 row samples, the 65th alone in its block
        N = 130 if name == "Z1" else 65
        F = forest_of(_random_forest(rng, N, 60 if name == "Z1" else 30, 5, chain_frac=0.2))
        last = F.add([0, 63, N - 1], -1, 0)
        pat = F.pat()
        pairs = [(last, 1, 2)] + light_pairs(rng, range(1, last), [1], 10)
        row, col = make_parts(rng, pat, N, _one_sample_part(), 1, pairs, private=(100, 5))
        return Case(name, row, col, pairs)
    # a part against itself: every k-mer is shared with itself, C is the diagonal of the patterns' k-mer counts
    pat = _random_forest(rng, 300, 200, 8, chain_frac=0.3)
    kmers = _universe(rng, 900)
    part = Part(pat, 300, kmers, rng.integers(1, 200, size=kmers.size))
    return Case(name, part, part, [])


BUILDERS = {
    "S": case_s, "C": case_c,
    "K1": lambda: _key_case("K1", 1710, 300, 512, 260, 511, 600),
    "K2": lambda: _key_case("K2", 1711, 70, 2, 200, 256, 60),
    "E2047": lambda: _sort_case("E2047", 1720, 23, 89, False),
    "E2048": lambda: _sort_case("E2048", 1721, 32, 64, True),
    "E2050": lambda: _sort_case("E2050", 1722, 41, 50, False),
    "P": lambda: _pool_case("P", 1740, 8255, 4159),
    "Ps": lambda: _pool_case("Ps", 1740, 520, 260),
    "Z0": lambda: _degenerate_case("Z0"), "Z1": lambda: _degenerate_case("Z1"), "Z2": lambda: _degenerate_case("Z2"),
    "Zself": lambda: _degenerate_case("Zself"),
}
NAMES = tuple(BUILDERS)
POOL_FACTOR = 1.3                                       # P's block records over the slots of the first pool
ORACLE_BUDGET = 1 << 25                                 # cell additions the CPU oracle is asked for per case (S: 10 M; P: 65 M)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def csr_of(dense):
    """(row_ptr, col, val) of the non-zeros of a dense cell, columns ascending inside a row"""
    r, c = np.nonzero(dense)
    row_ptr = np.zeros(dense.shape[0] + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(r, minlength=dense.shape[0]))
    return row_ptr, c, dense[r, c]


def tiles_of(dense):
    """the 64 x 64 tiles of a dense cell that hold a non-zero"""
    r, c = np.nonzero(dense)
    return int(np.unique((r // 64) * ((dense.shape[1] + 63) // 64) + c // 64).size)
