"""Inputs and references of test_all2all_rows.py: pattern forests that hold the edges of the band path on purpose (a band that ends inside a
local list, a node selected without a row, root paths of 63 / 64 / 65 / 130 nodes, lists either side of the LDS stack, ids and deltas beyond
2^16, subtree weights that wrap), the band of the matrix from the definition in numpy, and a host census of what the apply kernel does.

A forest is the dict of tensors synth.build_patterns returns (variant_cases._Forest builds it): pattern 0 is the empty pattern, a parent has a
smaller index than its children, ids ascend along a root path."""
import numpy as np

import gamma_cases as GC
import variant_cases as VC


def tri(i):
    return i * (i - 1) // 2 if i else 0


# ------------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------------
def band_definition(pat, N, lo, hi):
    """Rows [lo, hi) of all2all from the definition, flat form (variant_cases.definition restricted to those rows): every pattern with a
    weight adds it to the cells (i, j), j in front of i in its full list, of the ids i of the band.  Cell (i, j) at tri(i) - tri(lo) + j;
    uint32 arithmetic wraps around."""
    w = pat["num_kmers"].numpy()
    exp = np.zeros(tri(hi) - tri(lo), dtype=np.uint32)
    for p, full in enumerate(VC.full_lists(pat)):
        if w[p] == 0 or full.size < 2:
            continue
        assert (np.diff(full) > 0).all() and full[-1] < N, p
        a, b = np.searchsorted(full, lo), np.searchsorted(full, hi)
        for t in range(max(a, 1), b):
            i = int(full[t])
            exp[tri(i) - tri(lo) + full[:t]] += np.uint32(w[p])
    return exp


def census(pat, lo, hi):
    """What the apply launch does for the band, counted on the host: (nodes_applied, updates).  A node counts when it can add anything at all
    — local ids of its own, a column to pair them with (two ids or more in its full list), a subtree weight that is not 0 modulo 2^32 — and
    has a local id inside the band; it issues, for every such id, one addition per id in front of it in its full list (its position)."""
    par = pat["parent"].numpy()
    w = pat["num_kmers"].numpy().astype(np.uint64)
    n = pat["num_samples"].numpy()
    l = pat["num_local"].numpy()
    lp, ids = pat["local_ptr"].numpy(), pat["local_ids"].numpy()
    P = len(par)
    W = w.copy()
    for p in range(P - 1, 0, -1):                                   # a parent has a smaller index than its children
        if par[p] >= 0:
            W[par[p]] += W[p]
    ok = (l > 0) & (n > 1) & ((W & np.uint64(0xFFFFFFFF)) != 0)
    node = np.repeat(np.arange(P), l)
    pos = (n - l)[node] + (np.arange(ids.size) - lp[node])          # position of every local id in its node's full list
    m = ok[node] & (ids >= lo) & (ids < hi)
    return int(np.unique(node[m]).size), int(pos[m].sum())


def pat_of_host(h):
    """the forest of a HostDB: its view's arrays with every local list decoded by the test coder (gamma_cases.decode)"""
    import torch
    v = h.view_arrays()
    P = v["num_kmers"].size
    locs = []
    for p in range(P):
        nb, ln, off = int(v["num_bits"][p]), int(v["num_local"][p]), int(v["data_offset"][p])
        words = v["data"][off: off + (nb + 127) // 128 * 2]                 # (a list of one id has no stream)
        locs.append(np.asarray(GC.decode(words, nb, ln, int(v["last_sample_id"][p])), dtype=np.int64))
    nloc = np.array([x.size for x in locs], dtype=np.int64)
    assert np.array_equal(nloc, v["num_local"].astype(np.int64))
    lptr = np.zeros(P + 1, dtype=np.int64)
    lptr[1:] = np.cumsum(nloc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64)))      # noqa: E731
    return {"num_kmers": t(v["num_kmers"] & 0xFFFFFFFF), "parent": t(v["parent_id"]), "num_samples": t(v["num_samples"]), "num_local": t(nloc),
            "local_ptr": t(lptr), "local_ids": t(np.concatenate(locs) if locs else np.zeros(0, np.int64))}


def seeded_cuts(N, seed, k):
    """0 = r_0 < ... < r_k = N"""
    rng = np.random.default_rng(seed)
    inner = np.sort(rng.choice(np.arange(1, N), size=min(k - 1, N - 1), replace=False))
    return [0] + [int(x) for x in inner] + [N]


# ------------------------------------------------------------------------------------------------------------------------------------
# forests: (pat, N)
# ------------------------------------------------------------------------------------------------------------------------------------
def tiny_forest():
    """N = 9: two roots, a chain of depth 4 (0 1 | 2 | 4 5 | 8), siblings at two levels, the empty pattern 0"""
    F = VC._Forest()
    r1 = F.add([0, 1], -1, 3)
    c1 = F.add([2], r1, 5)
    c2 = F.add([4, 5], c1, 2)
    F.add([8], c2, 7)
    F.add([3, 6], r1, 1)
    F.add([7], c1, 4)
    r2 = F.add([1, 3, 7], -1, 6)
    F.add([8], r2, 9)
    return F.pat(), 9


def cut_forest():
    """a node with the local ids 3 .. 20 under a parent with 0 .. 2"""
    F = VC._Forest()
    r = F.add([0, 1, 2], -1, 2)
    F.add(range(3, 21), r, 3)
    return F.pat(), 21


def superset_forest():
    """a node with the local ids {2, 50}: selected for the band [10, 20), no row in it; {5, 12} has one"""
    F = VC._Forest()
    r = F.add([0, 1], -1, 1)
    F.add([2, 50], r, 4)
    F.add([5, 12], -1, 2)
    return F.pat(), 51


def chain_forest(depth, siblings):
    """a chain of `depth` nodes of one id each (N = depth); siblings: N - 1 more leaves of one id under the chain's middle node"""
    F = VC._Forest()
    N, par, mid = depth, -1, -1
    for i in range(depth):
        par = F.add([i], par, (1, 2, 127, 128, 3, 0, 255, 1)[i % 8])
        if i == depth // 2:
            mid = par
    if siblings:
        first = depth // 2 + 1
        for j in range(N - 1):
            F.add([first + (N - 1 - first - j) % (N - first)], mid, 1 + j % 5)
    return F.pat(), N


def long_list_forest(l):
    """a root with l local ids (a few gaps at the front), a child with two more behind them"""
    F = VC._Forest()
    ids = [0, 2, 5, 6, 9] + list(range(10, 10 + l - 5))
    r = F.add(ids, -1, 3)
    F.add([ids[-1] + 1, ids[-1] + 3], r, 2)
    return F.pat(), ids[-1] + 4


def deep_forest():
    """a chain of 4097 nodes of one id each, a leaf with the three ids left under it: N = 4100, a full list of 4100 ids"""
    F = VC._Forest()
    par = -1
    for i in range(4097):
        par = F.add([i], par, 1 + i % 7)
    F.add([4097, 4098, 4099], par, 5)
    return F.pat(), 4100


def wide_code_forest():
    """N = 70 002: a list that jumps from 0 to 69 999 (a delta of 2^16 and more: a code of 33 bits), patterns over ids above 66 000"""
    F = VC._Forest()
    F.add([0, 69999, 70000, 70001], -1, 5)
    r = F.add([66001, 66500, 70000], -1, 7)
    F.add([70001], r, 11)
    F.add(list(range(66000, 66100, 9)) + [70001], -1, 2)
    F.add([3, 70000], -1, 13)
    q = F.add([66010, 67000], -1, 0)
    F.add([68000, 70000, 70001], q, (1 << 32) - 1)
    return F.pat(), 70002


def weight_forest():
    """subtree sums that wrap past 2^32 (to 4, and to exactly 0: a node whose subtree adds nothing), a zero-weight node above children with a
    weight, a subtree without any weight"""
    F = VC._Forest()
    a = F.add([0, 1], -1, (1 << 32) - 1)
    F.add([2, 5], a, 5)
    b = F.add([1, 3], -1, (1 << 32) - 5)
    F.add([4], b, 5)
    z = F.add([0, 2], -1, 0)
    F.add([3], z, 3)
    F.add([6, 7], z, (1 << 31))
    F.add([7], z, (1 << 31))
    n = F.add([3, 4], -1, 0)
    F.add([5, 6], n, 0)
    return F.pat(), 8


def huge_forest():
    """N = 500 000: the triangle is half a terabyte; two patterns reach the last row"""
    F = VC._Forest()
    r = F.add([1, 70000, 499998], -1, 3)
    F.add([499999], r, 4)
    F.add([0, 499999], -1, 9)
    return F.pat(), 500000
