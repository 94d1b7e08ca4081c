"""Inputs and references of test_sample_rows_conformance.py: lower triangles CRAFTED cell by cell for kmdb_sampled_from_dense_device (it takes
any matrix the caller wrote), placed on the constants of csrc/sample_rows.hip — the four 8-bit digits of the radix select, the float key of the
proxy, the narrowed threshold of sr_select_kernel, the 1024-entry chunks and 64-lane groups of sr_sort_rows_kernel — and censuses that prove on
the host what the cases hold.  Host only: no GPU.

The reference is never the device.  It is test_sample_rows_device.expected_rows: the sampler's order (score descending, then id ascending)
over kmdbh_metric on the whole crafted matrix.  A NaN score ranks below every number there, as in host_sampler.cpp's better(): that rule is
this project's own choice — the reference's comparison (sampler.h:45-50) is no order on NaN scores, so it has nothing to conform to.

A case is one matrix, the callers' k-mer counts, and the (criterion, count) calls made on it.  The crafted rows are HUB rows: samples 0, 63,
64, 65, one mid-range id that is no multiple of 64, and N - 1, so that a hub's symmetric row is read partly as a tile's row line and partly
as its column line, on both sides of tile edges and in the partial last tile.  A hub's neighbours are never hubs, so its row holds exactly the
crafted values; a sprinkling of cells between other samples touches further tiles.

  digit0        cells 4^e, e < 16: sixteen different top-8 bins; the cut is settled in the first pass
  digits12      cells 256 + t, t < 256: one top-8 bin, 128 top-16 prefixes, 256 keys (counts 100, 1 and N + 5)
  digit3        cells 2^23 + t, t < 256: keys 0xcb000000 .. 0xcb0000ff, one 24-bit prefix; the bracket of the band is not vacuous here
  equal         500 cells of value 7, count 5: one bin in all four passes, everything is a candidate, the host keeps the five lowest ids
  exact         rows of count - 1, count and count + 1 cells
  fc_pairs      cells 2^24 + 1 + 2m, m < 200: 101 float keys; the cut lies inside one
  fc_top        cells 0xFFFFFF00 + t, t < 256: the upper half rounds to 2^32 (finite); the cut lies inside that key
  fc_jaccard    a = b = 4 * 10^7, c = 3 * 10^7 + t, t < 40: 40 doubles on 22 float keys, one 24-bit prefix; jaccard, ani, and mash (negative keys)
  fc_edge       count-th cell 2^26 + 5 (rounds UP to 2^26 + 8) and a cell 2^26 - 62 (rounds DOWN to 2^26 - 64) that lies inside the 1e-6 band:
                without the 2^-22 term of the narrowed threshold the device would hold it back (derivation at the case)
  flip_d3       mash-query, every k-mer count 1: proxies -(2^23 + t), keys 0x34ffff00 .. 0x34ffffff; the best cell is the smallest ratio
  flip_fc       mash-query, every k-mer count 1, cells 2^24 + 1 + 2m
  rowlen        N = 2100 (33 tile rows, a last tile of 52): hub rows of 64, 65, 1024, 1025, 2048 and 2049 distinct cells, emitted whole and by half
  unrankable    k-mer counts of 0 beside non-zero cells: rows of one unrankable cell and four finite ones, rows of three unrankable cells"""
import functools

import numpy as np

from test_sample_rows_device import CRITERIA, expected_rows, full_part, pairs_of, proxy_of, rows_of  # noqa: F401  (the tests import them from here)

K_LEN = 18
SMALL_N = 600                                           # 10 tile rows of 64, a last tile of 24
ROWLEN_N = 2100
KEY_BEST = 0xFFFFFFFF                                   # SR_KEY_BEST

# The band a truncated row brackets its candidates with, relative to T, the row's count-th largest exact proxy.
# BAND_LO is what the header of sample_rows.hip promises: every cell within the margin of the filters (1e-6 relative) comes out.
# BAND_HI follows from the constants of sr_select_kernel, it is no measurement: the threshold is T rounded to float (2^-24), narrowed by
# 1e-6 + 2^-22, rounded down one float (2^-23), and a cell passes by its own float (2^-24):
#     1e-6 + 2^-22 + 2^-24 + 2^-23 + 2^-24 = 1e-6 + 2^-21 = 1.4769e-6 < 1.49e-6
BAND_LO = 1e-6
BAND_HI = 1.5e-6
assert 1e-6 + 2.0 ** -22 + 2.0 ** -24 + 2.0 ** -23 + 2.0 ** -24 < 1.49e-6 < BAND_HI


def flat(a, b):
    i, j = max(a, b), min(a, b)
    assert i > j >= 0
    return i * (i - 1) // 2 + j


def hubs_of(N):
    mid = N // 2 + 1
    assert mid % 64 and 65 < mid < N - 1
    return (0, 63, 64, 65, mid, N - 1)


class Case:
    def __init__(self, name, N, kmers, runs):
        self.name, self.N, self.runs = name, N, list(runs)
        self.kmers = np.broadcast_to(np.asarray(kmers, np.int64), (N,)).copy()
        self.tri = np.zeros(N * (N - 1) // 2, np.uint32)
        self.hubs = {}                                  # hub -> (neighbours, values)
        self.rng = np.random.default_rng(sum(name.encode()))
        self.others = np.setdiff1d(np.arange(N), hubs_of(N))

    def put(self, a, b, v):
        x = flat(a, b)
        assert self.tri[x] == 0 and 0 < v < 1 << 32
        self.tri[x] = v

    def hub(self, h, values, pick=None):
        """the row of hub h: `values` on len(values) neighbours that are no hubs (or on `pick`)"""
        nb = self.rng.permutation(self.others)[:len(values)] if pick is None else np.asarray(pick)
        assert len(nb) == len(values) and h in hubs_of(self.N) and not np.isin(nb, hubs_of(self.N)).any()
        for o, v in zip(nb.tolist(), values):
            self.put(h, o, int(v))
        self.hubs[h] = (nb, np.asarray(values, np.int64))

    def every_hub(self, values):
        """the same row on every hub; where the samples suffice the hubs share no neighbour, so that no other row holds two crafted cells"""
        n, perm = len(values), self.rng.permutation(self.others)
        for x, h in enumerate(hubs_of(self.N)):
            self.hub(h, values, pick=perm[x * n:(x + 1) * n] if 6 * n <= len(perm) else None)
        return self

    def sprinkle(self, n, hi):
        """n cells of value 1 .. hi between samples that are no hubs"""
        a = self.rng.choice(self.others, n)
        b = self.rng.choice(self.others, n)
        for x, y, v in zip(a.tolist(), b.tolist(), self.rng.integers(1, hi + 1, n).tolist()):
            if x != y and self.tri[flat(x, y)] == 0:
                self.put(x, y, v)
        return self


# ------------------------------------------------------------------------------------------------------------------------------------
# the key of the device, restated
# ------------------------------------------------------------------------------------------------------------------------------------
def key_of(p):
    """sr_key in numpy: the float32 bits of the proxy, the sign bit flipped for a positive and every bit for a negative number, so that the
    keys order as the numbers do; KEY_BEST for a proxy that is no finite float"""
    p = np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        f = p.astype(np.float32)
    u = f.view(np.uint32)
    key = np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000))
    return np.where(np.isfinite(p) & np.isfinite(f), key, np.uint32(KEY_BEST)).astype(np.uint32)


def settle_digit(keys, count):
    """the 8-bit pass (0 = the top bits) after which the count-th largest key of a row shares its prefix with no DIFFERENT key of the row —
    the last pass in which the radix select still tells keys apart; None: every key of the row is the same"""
    ks = np.sort(np.asarray(keys, np.uint32))[::-1]
    kc = ks[count - 1]
    other = np.unique(ks[ks != kc])
    if not other.size:
        return None
    top = np.floor(np.log2((other ^ kc).astype(np.float64))).astype(np.int64)         # the highest differing bit
    return int((3 - top // 8).max())


def count_inside_key(keys, start):
    """the first count >= start at which the cut falls inside one float key: the count-th and the (count + 1)-th largest key are the same"""
    ks = np.sort(np.asarray(keys, np.uint32))[::-1]
    for c in range(start, len(ks)):
        if ks[c - 1] == ks[c]:
            return c
    raise AssertionError("no two cells of the row share a key")


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------
def _small(name, kmers, runs, values, sprinkle_hi=50):
    return Case(name, SMALL_N, kmers, runs).every_hub(values).sprinkle(300, sprinkle_hi)


def _fc_jaccard():
    vals = 30_000_000 + np.arange(40)
    c = Case("fc_jaccard", SMALL_N, 40_000_000, []).every_hub(vals).sprinkle(300, 1000)
    p = vals / (80_000_000 - vals)
    up = count_inside_key(key_of(p), 3)                 # the best cells are the largest ratios
    down = count_inside_key(key_of(-p), 3)              # mash: the smallest
    assert up < 10 and down < 10
    c.runs = [("jaccard", up), ("ani", up), ("mash", down)]
    return c


def _exact(count=5):
    c = Case("exact", SMALL_N, 1000, [("num-kmers", count)])
    for h, n in zip(hubs_of(SMALL_N), (count - 1, count, count + 1) * 2):
        c.hub(h, 10 + 3 * np.arange(n))
    return c.sprinkle(300, 50)


def _rowlen():
    N = ROWLEN_N
    c = Case("rowlen", N, 5000 + np.arange(N) * 37 % 1000, [("num-kmers", 3000), ("num-kmers", 32), ("num-kmers", 512), ("num-kmers", 1024), ("jaccard", 512)])
    for h, n in zip(hubs_of(N), (2049, 64, 1025, 65, 2048, 1024)):
        vals = 1 + (np.arange(n) * 7919 + 13 * h) % 4099
        assert len(np.unique(vals)) == n
        c.hub(h, vals)
    c.put(1500, 7, 77)                                  # the one-cell range of RANGES
    return c.sprinkle(3000, 4000)


def _unrankable():
    """hub 63 / 0 / N - 1: one cell beside a sample of count 0 and of the hub's own count (a + b - c = 0), four finite cells;
    hub 64: three such cells and four finite ones; hub 65 and the mid hub have count 0 themselves and one / three neighbours of count 0
    (max is infinite only there; min, cosine and ani-shorter are on every cell of those rows)"""
    N = SMALL_N
    c = Case("unrankable", N, 2000 + np.arange(N) * 37 % 500, [(cr, 2) for cr in CRITERIA])
    h0, h63, h64, h65, mid, last = hubs_of(N)
    zeros = {h63: [110], h64: [100, 101, 102], h65: [120], mid: [mid + 30, mid + 31, mid + 32], h0: [140], last: [150]}
    for h, zs in zeros.items():
        c.kmers[h] = 0 if h in (h65, mid) else 500
        c.kmers[zs] = 0
        finite = [200 + 10 * x for x in range(4)]
        c.hub(h, [9 if h in (h65, mid) else 500] * len(zs) + [100, 200, 300, 400], pick=zs + finite)
    return c.sprinkle(300, 50)


def _fc_edge():
    """T = 2^26 + 5 is the 5th largest cell; as a float it is 2^26 + 8.  p = 2^26 - 62 lies inside the band (T * 1e-6 = 67.1: the band reaches
    down to 2^26 - 62.1) and as a float it is 2^26 - 64 (floats step by 4 below 2^26; the tie goes to the even mantissa).  Narrowed by 1e-6 alone
    the threshold would be 2^26 + 8 - 67.1 rounded down = 2^26 - 60 > 2^26 - 64: the cell would be held back.  With the 2^-22 term it is
    2^26 + 8 - 83.1 rounded down = 2^26 - 76.  2^26 - 100 lies below T (1 - 1.5e-6) = 2^26 - 95.7 and must stay behind."""
    B = 1 << 26
    vals = [B + 400, B + 300, B + 200, B + 100, B + 5, B - 62, B - 100, B - 200] + [1 << e for e in range(10, 25)]
    T, p = float(B + 5), float(B - 62)
    assert float(np.float32(T)) == B + 8 and float(np.float32(p)) == B - 64
    assert T - T * BAND_LO <= p and B - 100 < T - T * BAND_HI
    return _small("fc_edge", 1000, [("num-kmers", 5)], vals)


def _build():
    N = SMALL_N
    d3 = (1 << 23) + np.arange(256)
    pairs = (1 << 24) + 1 + 2 * np.arange(200)
    top = 0xFFFFFF00 + np.arange(256)
    cases = [
        _small("digit0", 1000, [("num-kmers", 5)], 4 ** np.arange(16)),
        _small("digits12", 1000, [("num-kmers", 100), ("num-kmers", 1), ("num-kmers", N + 5)], 256 + np.arange(256)),
        _small("digit3", 1000, [("num-kmers", 100)], d3),
        _small("equal", 1000, [("num-kmers", 5)], [7] * 500),
        _exact(),
        _small("fc_pairs", 1000, [("num-kmers", count_inside_key(key_of(pairs), 50))], pairs),
        _small("fc_top", 1000, [("num-kmers", count_inside_key(key_of(top), 60))], top),
        _fc_jaccard(),
        _fc_edge(),
        _small("flip_d3", 1, [("mash-query", 100)], d3),
        _small("flip_fc", 1, [("mash-query", count_inside_key(key_of(-pairs.astype(np.float64)), 50))], pairs),
        _rowlen(),
        _unrankable(),
    ]
    return {c.name: c for c in cases}


CASES = _build()
NAMES = list(CASES)

# flat ranges of the rowlen matrix that together cover its triangle: [row start, row end), one cell, inside one hub's triangle row, from the middle
# of a row inside a diagonal tile, up to the last cell
_T = lambda r: r * (r - 1) // 2                         # noqa: E731  (the first cell of triangle row r)
_MID = hubs_of(ROWLEN_N)[4]
RANGE_CUTS = [0, _T(130) + 129, _T(500), _T(900), _T(_MID) + 100, _T(_MID) + 700, flat(1500, 7), flat(1500, 7) + 1, _T(2000), _T(ROWLEN_N)]
assert RANGE_CUTS == sorted(set(RANGE_CUTS)) and 128 <= 129 < 130 < 192 and _MID > 700


# ------------------------------------------------------------------------------------------------------------------------------------
# the model of a call
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sym_rows(name, criterion):
    """the symmetric rows of a case in ascending columns: (ptr, col, val, exact proxy in double)"""
    c = CASES[name]
    i, j, v = pairs_of(c.tri, c.N)
    p = proxy_of(criterion, v, c.kmers[i], c.kmers[j])
    s = np.concatenate([i, j]); o = np.concatenate([j, i]); v = np.concatenate([v, v]); p = np.concatenate([p, p])
    order = np.lexsort((o, s))
    ptr = np.zeros(c.N + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(s, minlength=c.N))
    return ptr, o[order], v[order], p[order]


def hub_proxies(name, criterion, h):
    ptr, _, _, p = sym_rows(name, criterion)
    return p[ptr[h]:ptr[h + 1]]


@functools.lru_cache(maxsize=None)
def row_models(name, criterion, count):
    """per row what the candidates must be, and the rows that are truncated (cut with something left below the cut):
         ("whole", cols)          fewer than `count` cells, or a cell the device cannot rank: the row comes out whole
         ("cut", lo, hi, cols)    lo <= candidates <= hi, the sets of columns within BAND_LO / BAND_HI of T
       A cut row is truncated when hi is not the whole row and is not when lo is; no case has a row between the two (asserted here)."""
    ptr, col, _, p = sym_rows(name, criterion)
    out, truncated = [], 0
    for s in range(len(ptr) - 1):
        cs, ps = col[ptr[s]:ptr[s + 1]], p[ptr[s]:ptr[s + 1]]
        if len(cs) < count or (key_of(ps) == KEY_BEST).any():
            out.append(("whole", cs))
            continue
        T = np.sort(ps)[::-1][count - 1]
        lo, hi = cs[ps >= T - abs(T) * BAND_LO], cs[ps >= T - abs(T) * BAND_HI]
        assert len(hi) < len(cs) or len(lo) == len(cs), (name, criterion, count, s)
        truncated += len(hi) < len(cs)
        out.append(("cut", lo, hi, cs))
    return out, truncated


_EXPECTED = {}


def expected(K, name, criterion, count):
    key = (name, criterion, count)
    if key not in _EXPECTED:
        c = CASES[name]
        _EXPECTED[key] = expected_rows(K, c.tri, c.N, c.kmers, K_LEN, criterion, count)
    return _EXPECTED[key]


# ------------------------------------------------------------------------------------------------------------------------------------
# censuses: what the cases hold, on the host
# ------------------------------------------------------------------------------------------------------------------------------------
def census_digits():
    """per digit case and hub row: the pass that settles the cut, and the key patterns the case is named for"""
    N = SMALL_N
    for name, criterion, count, digit in (("digit0", "num-kmers", 5, 0), ("digits12", "num-kmers", 100, 2), ("digits12", "num-kmers", 1, 2),
                                          ("digit3", "num-kmers", 100, 3), ("flip_d3", "mash-query", 100, 3), ("equal", "num-kmers", 5, None)):
        for h in hubs_of(N):
            assert settle_digit(key_of(hub_proxies(name, criterion, h)), count) == digit, (name, h)
    k = key_of(hub_proxies("digit0", "num-kmers", 0))
    assert len(np.unique(k >> np.uint32(24))) == 16
    k = key_of(hub_proxies("digits12", "num-kmers", 63))
    assert len(np.unique(k)) == 256 and len(np.unique(k >> np.uint32(16))) == 128 and len(np.unique(k >> np.uint32(24))) == 1
    k = np.sort(key_of(hub_proxies("digit3", "num-kmers", 64)))
    assert k[0] == 0xcb000000 and k[-1] == 0xcb0000ff and len(np.unique(k)) == 256
    k = np.sort(key_of(hub_proxies("flip_d3", "mash-query", 65)))
    assert k[0] == 0x34ffff00 and k[-1] == 0x34ffffff and len(np.unique(k)) == 256
    k = key_of(hub_proxies("equal", "num-kmers", N - 1))
    assert len(k) == 500 and len(np.unique(k)) == 1
    assert settle_digit(np.array([KEY_BEST]), 1) is None and CASES["digits12"].runs[2][1] > N
    assert sorted(len(CASES["exact"].hubs[h][0]) for h in hubs_of(N)) == [4, 4, 5, 5, 6, 6] and CASES["exact"].runs == [("num-kmers", 5)]


def census_collapse():
    """the float-collapse rows: fewer keys than doubles, the cut inside one key, and what the flipped criteria rank by"""
    for name, criterion, doubles, keys in (("fc_pairs", "num-kmers", 200, 101), ("fc_top", "num-kmers", 256, 2), ("flip_fc", "mash-query", 200, 101),
                                           ("fc_jaccard", "jaccard", 40, 22), ("fc_jaccard", "mash", 40, 22), ("fc_jaccard", "ani", 40, 22)):
        count = dict(CASES[name].runs)[criterion]
        for h in hubs_of(SMALL_N):
            p = hub_proxies(name, criterion, h)
            k = np.sort(key_of(p))[::-1]
            assert len(np.unique(p)) == doubles and len(np.unique(k)) == keys, (name, len(np.unique(k)))
            assert k[count - 1] == k[count] and k.max() != KEY_BEST, name
            assert (k < 0x80000000).all() == (criterion in ("mash", "mash-query"))                       # the flipped criteria: negative keys
            if name == "fc_jaccard":
                assert settle_digit(k, count) == 3                                                       # and one 24-bit prefix
    top = key_of(hub_proxies("fc_top", "num-kmers", 0))
    assert top.max() == key_of([2.0 ** 32])[0] and np.count_nonzero(top == top.max()) == 128


def census_bracket():
    """the bracket is not vacuous: in the digit-3 rows the sets within BAND_LO and BAND_HI differ (cells >= T - 8 and >= T - 12), the model holds a
    truncated and a whole row in every case that cuts, and fc_edge's cell is inside the lower band"""
    rows, truncated = row_models("digit3", "num-kmers", 100)
    for h in hubs_of(SMALL_N):
        kind, lo, hi, cs = rows[h]
        T = (1 << 23) + 255 - 99
        nb, vals = CASES["digit3"].hubs[h]
        assert kind == "cut" and set(lo) == set(nb[vals >= T - 8].tolist()) and set(hi) == set(nb[vals >= T - 12].tolist()) and len(lo) + 4 == len(hi)
    assert truncated >= 6
    rows, _ = row_models("fc_edge", "num-kmers", 5)
    nb, vals = CASES["fc_edge"].hubs[63]
    assert int(nb[vals == (1 << 26) - 62][0]) in rows[63][1] and int(nb[vals == (1 << 26) - 100][0]) not in rows[63][2]
    for name in NAMES:
        for criterion, count in CASES[name].runs:
            row_models(name, criterion, count)          # (asserts that no row lies between the two bands)


def census_rowlen():
    c = CASES["rowlen"]
    ptr = sym_rows("rowlen", "num-kmers")[0]
    assert [int(ptr[h + 1] - ptr[h]) for h in hubs_of(c.N)] == [2049, 64, 1025, 65, 2048, 1024]
    assert (c.N + 63) // 64 == 33 and c.N - 32 * 64 == 52 and 20_000 > np.count_nonzero(c.tri) > 8_000
    assert row_models("rowlen", "num-kmers", 3000)[1] == 0
    for count, h in ((32, 63), (512, 64), (1024, 0)):   # about half of a hub's row
        kind, lo, hi, cs = row_models("rowlen", "num-kmers", count)[0][h]
        assert kind == "cut" and len(lo) == len(hi) == count and len(cs) in (2 * count, 2 * count + 1)


def census_unrankable():
    """for every criterion but num-kmers (whose proxy is the cell) a row with ONE unrankable cell and >= 3 finite ones, and a row with >= count"""
    for criterion, count in CASES["unrankable"].runs:
        ptr, _, _, p = sym_rows("unrankable", criterion)
        bad = np.add.reduceat((~np.isfinite(np.append(p, 0.0))).astype(np.int64), ptr[:-1])
        bad[np.diff(ptr) == 0] = 0
        n = np.diff(ptr)
        if criterion == "num-kmers":
            assert not bad.any()
            continue
        assert ((bad == 1) & (n - bad >= 3)).any() and ((bad >= count) & (n - bad >= 3)).any(), criterion
