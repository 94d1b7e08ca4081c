"""Inputs of test_decode_order.py: explicit forests of at most 200 samples for the short decode launch's work order.  Host only.

Every node but one is a root, and roots keep their pattern order in the DFS layout (children are grouped by parent, pattern order inside a
family), so node i of the layout is pattern i here: a forest decides what every window of W consecutive nodes holds.  Pattern 0 is the empty
pattern every database has (l == 0: nothing to decode, but its entry is the short launch's to write: key 1).

The kinds of lists, by what the order's key (kmdb_k0_key: l, stream bits, KMDB_SHORT_IDS) makes of them:
  single    l == 1 (and the empty list: its zero is written)    key 1, no stream
  run       l consecutive ids: l - 1 deltas of 1 in l - 1 bits   key 2, no stream word read
  coded     deltas above 1: 2 + the bits beyond one per delta    key 2 + extra, capped at 63
  long      more than KMDB_SHORT_IDS ids, or more than 128 bits  key 0 (the long launch's)
A delta of L bits costs 2 L - 1 stream bits, 2 L - 2 beyond its one: the extra bits of a list are EVEN, and a list of l ids has l - 1 + extra
bits — the same parity as l - 1.  So the keys at the cap are made from extras of 58 .. 66 in steps of two (62 and 64 among them; no list has 63),
and the lists either side of the 128-bit test are 47 ids in 128 / 130 bits and 48 ids in 127 / 129 bits (48 ids in 128 bits do not exist).
"""
import functools

import numpy as np

import variant_cases as V

N = 200
WINDOWS = (256, 1024, 4096)


def single(i):
    return [i % N]


def run(i, l):
    first = (7 * i) % (N - l + 1)
    return list(range(first, first + l))


def from_deltas(i, deltas):
    first = (5 * i) % (N - sum(deltas))
    return [first] + [first + int(s) for s in np.cumsum(deltas)]


def twos(i, n_twos, n_ones=0):
    """a coded list: n_twos deltas of 2 (extra bits 2 each) and n_ones deltas of 1, spread among them"""
    deltas = [2] * n_twos
    for k in range(n_ones):
        deltas.insert((k * 3) % (len(deltas) + 1), 1)
    return from_deltas(i, deltas)


def heavy(i):
    """48 ids in 93 bits, 23 codes that are not "0" each behind a "0": a decode step per code, the most steps of the lists here"""
    return from_deltas(i, [2, 1, 3, 1] * 11 + [2, 1, 1])


def long_run(i):
    return run(i, 49 + i % 3)                                   # (short again under KMDB_SHORT_IDS=64)


def long_bits(i):
    return twos(i, 42, 3)                                       # 46 ids, 45 + 84 = 129 bits: long at every KMDB_SHORT_IDS


def header(ids):
    """(l, stream bits) of a list"""
    d = np.diff(np.asarray(ids, dtype=np.int64))
    return len(ids), int(sum(2 * int(x).bit_length() - 1 for x in d))


def key_of(l, nbits, short_ids=48):
    """the order's key, written from DESIGN.md's rule (not from the engine's source)"""
    if l > short_ids or nbits > 128:
        return 0
    if l <= 1:
        return 1
    extra = nbits - (l - 1)
    return 2 if extra == 0 else min(2 + extra, 63)


SHAPES = (
    ("run l=2", lambda i: run(i, 2)), ("run l=48", lambda i: run(i, 48)), ("run l=47", lambda i: run(i, 47)), ("l=49", lambda i: run(i, 49)),
    ("47 ids 128 bits", lambda i: twos(i, 41, 5)), ("47 ids 130 bits", lambda i: twos(i, 42, 4)),
    ("48 ids 127 bits", lambda i: twos(i, 40, 7)), ("48 ids 129 bits", lambda i: twos(i, 41, 6)),
    ("extra 58", lambda i: twos(i, 29, i % 4)), ("extra 60", lambda i: twos(i, 30, i % 3)), ("extra 62", lambda i: twos(i, 31, i % 5)),
    ("extra 64", lambda i: twos(i, 32)), ("extra 66", lambda i: twos(i, 33, 2)), ("extra 62, deltas of 4", lambda i: from_deltas(i, [4] * 15 + [2])),
    ("heavy", heavy), ("single", single), ("two ids far apart", lambda i: [i % 50, 150 + i % 50]), ("long bits", long_bits),
    ("run over blocks", lambda i: run(i, 40 + i % 9)),          # with a block width of 32: one or two block boundaries inside the run
    ("coded short", lambda i: from_deltas(i, [1, 1, 5, 1, 2, 1, 1, 9])),
)


def mixed_forest(P):
    """P patterns in all: the empty one, then the shapes in turn with singles and runs thrown in (every wave mixes lists that read their stream
    with lists that do not), one child under pattern 1 so that a root path exists"""
    F = V._Forest()
    for i in range(1, P):
        if i == 2:
            F.add([180, 199], 1, 3)                              # (pattern 1 is the run of 48 ids from id 7)
            continue
        k = i % (len(SHAPES) + 7)
        ids = SHAPES[k][1](i) if k < len(SHAPES) else (single(i) if k % 2 else run(i, 2 + i % 30))
        F.add(ids, -1, 1 + i % 5)
    return F.pat()


def window_forest(W):
    """windows of W nodes by content -> (forest, {name: window index}).  0: the empty pattern and W - 1 singles; 1: singles alone; 2: runs alone;
    3: long nodes alone; 4: long nodes and ONE decodable node (at offset 77); 5: singles and runs with 64 heavy nodes among them (every W / 64-th);
    6, part-filled: the shapes in turn"""
    F = V._Forest()
    fill = [("singles0", lambda i, o: single(i)), ("singles", lambda i, o: single(i)), ("runs", lambda i, o: run(i, 2 + i % 47)),
            ("long", lambda i, o: long_run(i) if i % 2 else long_bits(i)),
            ("one", lambda i, o: heavy(i) if o == 77 else (long_run(i) if i % 2 else long_bits(i))),
            ("heavy64", lambda i, o: heavy(i) if o % (W // 64) == 3 % (W // 64) else (single(i) if i % 3 else run(i, 2 + i % 40)))]
    names = {}
    for w, (name, make) in enumerate(fill):
        names[name] = w
        for o in range(W):
            i = w * W + o
            if i:
                F.add(make(i, o), -1, 1 + i % 4)
    names["shapes"] = len(fill)
    for o in range(3 * len(SHAPES) + 5):
        i = len(fill) * W + o
        F.add(SHAPES[o % len(SHAPES)][1](i), -1, 1 + i % 4)
    return F.pat(), names


def node_counts(W):
    return sorted({1, 63, 64, 65, 255, 256, 257, W - 1, W, W + 1, 2 * W + 5})


@functools.lru_cache(maxsize=None)
def mixed_case(P):
    """(forest, definition): computed once, shared, never written to"""
    pat = mixed_forest(P)
    exp = V.definition(pat, N)
    exp.setflags(write=False)
    return pat, exp


@functools.lru_cache(maxsize=None)
def window_case(W):
    pat, names = window_forest(W)
    exp = V.definition(pat, N)
    exp.setflags(write=False)
    return pat, names, exp


def check_order(W, P, order, live, l, nbits, short_ids=48):
    """every window's offsets are a permutation of its slots, the keys along them do not increase (slots behind node P - 1: key 0), and the live
    count is the number of nodes with a key above 0.  -> keys in DFS order"""
    n_win = (P + W - 1) // W
    assert order.shape == (n_win, W) and live.shape == (n_win,) and l.shape == (P,)
    keys = np.zeros(n_win * W, dtype=np.int64)
    keys[:P] = [key_of(int(a), int(b), short_ids) for a, b in zip(l, nbits)]
    keys = keys.reshape(n_win, W)
    assert np.array_equal(np.sort(order, axis=1), np.broadcast_to(np.arange(W), (n_win, W))), "a permutation per window"
    along = np.take_along_axis(keys, order.astype(np.int64), axis=1)
    assert (np.diff(along, axis=1) <= 0).all(), "keys do not increase"
    assert np.array_equal(live, (keys > 0).sum(axis=1)), (live, (keys > 0).sum(axis=1))
    return keys
