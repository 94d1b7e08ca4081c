"""Inputs and references of test_kernel_variants.py: pattern forests that hold the edges of the first-block kernels on purpose, the
flat-form definition of all2all in numpy, a host census of the first-block records — and a __main__ for the engine's switches that are
read once per process (static locals of blocks_attempt), which an in-process test cannot set: test_kernel_variants.py starts
`python tests/variant_cases.py <label>` with the switches in the child's environment.

A forest is the dict of tensors synth.build_patterns returns (num_kmers, parent, num_samples, num_local, local_ptr, local_ids); pattern 0
is the empty pattern, a parent has a smaller index than its children, ids ascend along a root path."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = (32, 33, 50, 54, 55, 63, 64)
# either side of the int8 operand limit (127 | 128), of 8 / 16 / 31 / 32 bits, and 0 (a pattern without k-mers adds nothing)
WEIGHTS = (1, 2, 126, 127, 128, 129, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 0)


def edge_sizes(width):
    """the two sample counts of an edge forest: a last block of one sample, a last block short by one"""
    return (3 * width + 1, 4 * width - 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# forests
# ------------------------------------------------------------------------------------------------------------------------------------
class _Forest:
    def __init__(self):
        self.locs, self.parent, self.w = [np.zeros(0, dtype=np.int64)], [-1], [0]

    def add(self, ids, parent, w):
        ids = np.asarray(sorted(set(int(i) for i in ids)), dtype=np.int64)
        assert ids.size > 0
        if parent >= 0:
            q = parent
            while self.locs[q].size == 0:
                q = self.parent[q]
            assert ids[0] > self.locs[q][-1], "ids ascend along a root path"
        self.locs.append(ids); self.parent.append(parent); self.w.append(int(w))
        return len(self.locs) - 1

    def pat(self):
        import torch
        P = len(self.locs)
        nloc = np.array([len(x) for x in self.locs], dtype=np.int64)
        nsam = np.zeros(P, dtype=np.int64)
        for p in range(1, P):
            nsam[p] = nloc[p] + (nsam[self.parent[p]] if self.parent[p] >= 0 else 0)
        lp = np.zeros(P + 1, dtype=np.int64)
        lp[1:] = np.cumsum(nloc)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64)))      # noqa: E731
        return {"num_kmers": t(self.w), "parent": t(self.parent), "num_samples": t(nsam), "num_local": t(nloc), "local_ptr": t(lp),
                "local_ids": t(np.concatenate(self.locs))}


def edge_forest(width, N):
    """A deterministic forest over N samples whose blocks of `width` ids hold, for every block X: one-block nodes of every weight of WEIGHTS
    with masks of 1, 2 and all ids and with ids at positions 0 / 31 / 32 / width - 1 (the rows and columns either side of the 32 / 32
    split of the matrix-core tile); two-block nodes (a parent in X, children that add ids in every block Y > X: the second-block records
    (Y, X) and (Y, Y)), a local list over two blocks, nodes with three and four blocks (the wide kernel's, parents carried along); a
    chain of one-id nodes through the block and a fan of 135 leaves under its first node (a chain slot read two batches of 64 after it
    was written); and root subtrees of one to three nodes whose first blocks cycle, so that every slice of 64 DFS nodes there changes
    its first block many times and meets the same block again.  One chain of one-id nodes runs through ALL samples (a root path of N
    nodes: a block of at most 64 ids cannot hold a chain of more than 64, so the chain longer than two batches leaves its first block —
    its nodes with more than two blocks are the wide kernel's)."""
    assert 32 <= width <= 64 and N > 2 * width
    NB = (N + width - 1) // width
    lo = lambda X: X * width                                    # noqa: E731
    size = lambda X: min(width, N - X * width)                  # noqa: E731
    at = lambda X, pos: [lo(X) + p for p in sorted(set(pos)) if 0 <= p < size(X)]      # noqa: E731
    F = _Forest()
    for X in range(NB):
        bs = size(X)
        masks = [at(X, [0]), at(X, [0, bs - 1]), at(X, range(bs)), at(X, [0, 31, 32, width - 1, bs - 1])]
        for k, w in enumerate(WEIGHTS):
            for m in masks:
                F.add(m, -1, w)
            # the split rows one by one: (31, 32), (0, 31), (32, width - 1) and a column of the lower-right quarter alone
            F.add(at(X, [31, 32][: 1 + k % 2] + [k % bs]), -1, w)
            F.add(at(X, [32, 33 + k % 20, bs - 1]), -1, w)
    heavy = (1, 127, 128, 255, 65536, (1 << 32) - 1)
    for X in range(NB):
        par = F.add(at(X, [0, 31, size(X) - 1]), -1, 5)
        for Y in range(X + 1, NB):
            c = F.add(at(Y, [0, 32, size(Y) - 1]), par, heavy[(X + Y) % 6])          # (Y, X) and, with two ids in Y, (Y, Y)
            F.add(at(Y, [1]) or at(Y, [0]), par, heavy[(X + Y + 3) % 6])                 # one id in Y: (Y, X) alone
            for Z in range(Y + 1, NB):                                                   # three blocks and more: the wide kernel's
                g = F.add(at(Z, [0, size(Z) - 1]), c, heavy[(Y + Z) % 6])
                if Z + 1 < NB:
                    F.add(at(Z + 1, [0]), g, 127 + (Z & 1))
        if X + 1 < NB:
            F.add(at(X, [1, size(X) - 1]) + at(X + 1, [0, 1]), -1, 128 - (X & 1))       # a local list over two blocks
    for X in range(NB):
        bs = size(X)
        par, first = -1, -1
        for p in range(bs):                                                              # chain inside the block
            par = F.add([lo(X) + p], par, (1, 2, 127, 128, 3, 0, 255)[p % 7])
            first = par if p == 0 else first
        if bs >= 3:
            for j in range(135):                                                         # fan: three batches of leaves under one slot of the chain table
                a, b = 1 + j % (bs - 1), 1 + (j // (bs - 1) + 2 * j + 1) % (bs - 1)
                F.add([lo(X) + a, lo(X) + b], first, (1, 3, 127, 128, 2, 200)[j % 6])
    cyc = [X for X in range(NB) if size(X) >= 4]
    for t in range(150):                                                                 # first blocks cycle X, Y, Z, X, ...
        X = cyc[(t + t // 9) % len(cyc)]                                                 # (+ t // 9: the subtree's size does not follow its block)
        bs = size(X)
        a = t % (bs - 3)
        r = F.add([lo(X) + a, lo(X) + a + 1 + t % 2], -1, (1, 127, 128, 2, 126, 129, 7)[t % 7])
        if t % 3 >= 1:
            c = F.add([lo(X) + a + 3 + (t % 5) % (bs - a - 3)], r, (3, 128, 127, 1)[t % 4])
            later = [Y for Y in cyc if Y > X]
            if t % 3 == 2 and later:                                                     # a second block below: (Y, X), (Y, Y)
                Y = later[t % len(later)]
                F.add(at(Y, [t % size(Y), size(Y) - 1]), c, 1 + t % 130)
            elif t % 3 == 2 and F.locs[c][-1] < N - 1:
                F.add([N - 1], c, 1 + t % 130)
    par = -1
    for i in range(N):                                                                   # the chain through all samples
        par = F.add([i], par, (1, 2, 127, 128, 3, 0, 255, 1)[i % 8])
    return F.pat()


def light_forest(width, N):
    """Every weight below 128 and no record (Y, Y) of a second block: the diagonal tiles get first-block records of the matrix-core step
    only, so that a tile is flagged as touched — all2all-sp scans no other — by the kernel that applies those (dflush of k1n_kernel<1>,
    the flush of k2d_kernel, k2_apply_kernel) or not at all.  One-block roots whose blocks cycle, every fifth with a child of ONE id in a
    later block (the record (Y, X): an off-diagonal tile)."""
    NB = (N + width - 1) // width
    size = lambda X: min(width, N - X * width)                  # noqa: E731
    full = [X for X in range(NB) if size(X) >= 4]
    F = _Forest()
    for t in range(260):
        X = full[(t + t // 11) % len(full)]
        bs = size(X)
        pos = sorted({t % bs, (31 + t) % bs, (32 + 3 * t) % bs} if t % 4 else {0, 31, 32 % bs, bs - 1})
        r = F.add([X * width + p for p in pos], -1, (1, 2, 126, 127, 3)[t % 5])
        if t % 5 == 0 and X + 1 < NB:
            Y = X + 1 + t % (NB - X - 1)
            F.add([Y * width + t % size(Y)], r, (127, 1, 5)[t % 3])
    return F.pat()


def decode_forest(N=4096):
    """Local lists of exactly 1, 2, 47, 48, 49, 63, 64, 65 and 128 ids — either side of the 48 ids up to which the short launch of the decode
    kernel takes a list (KMDB_SHORT_IDS moves that boundary), of one wave and of two — in three delta shapes: all deltas 1; deltas
    2^j - 1 and 2^j, j = 1 .. 11 (where the Elias-gamma code changes its length; as many of them as the id range holds, the lists start at
    different j); the first id as small and the last id as large (N - 1) as they can be.  Every list once as a root and once under a parent
    of 40 ids."""
    F = _Forest()
    parent_ids = list(range(0, 80, 2))
    par = F.add(parent_ids, -1, 3)
    D = [d for j in range(1, 12) for d in ((1 << j) - 1, 1 << j)]
    n = 0
    for L in (1, 2, 47, 48, 49, 63, 64, 65, 128):
        for under in (False, True):
            base = parent_ids[-1] + 1 if under else 0
            room = N - 1 - base
            shapes = [[base + 5 * (n % 7) + i for i in range(L)]]
            ids, k = [base + n % 3], 3 * n
            for i in range(L - 1):
                d = D[k % len(D)]
                k += 1
                if ids[-1] + d + (L - 2 - i) > N - 1:
                    d = 1
                ids.append(ids[-1] + d)
            shapes.append(ids)
            shapes.append([N - 1] if L == 1 else sorted(set(base + int(round(x)) for x in np.linspace(0, room, L))))
            for ids in shapes:
                assert len(ids) == L and ids[-1] < N
                F.add(ids, par if under else -1, 1 + n % 5)
                n += 1
    return F.pat()


# ------------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------------
def full_lists(pat):
    """per pattern its full list (local ids plus the parents'), ascending"""
    par = pat["parent"].numpy()
    lp, ids = pat["local_ptr"].numpy(), pat["local_ids"].numpy()
    full = []
    for p in range(len(par)):
        loc = ids[lp[p]: lp[p + 1]]
        full.append(loc if par[p] < 0 else np.concatenate([full[par[p]], loc]))
    return full


@functools.lru_cache(maxsize=None)
def _tril(n):
    return np.tril_indices(n, -1)


def definition(pat, N, dtype=np.uint32):
    """all2all from the definition, flat form (reference similarity_calculator.cpp:596-638): every pattern with a non-zero weight adds its
    weight to all pairs of its full list.  Lower triangle, cell (i, j), j < i, at i (i - 1) / 2 + j; uint32 arithmetic wraps around
    (dtype=np.uint64: the exact sums)."""
    w = pat["num_kmers"].numpy()
    exp = np.zeros(N * (N - 1) // 2, dtype=dtype)
    for p, full in enumerate(full_lists(pat)):
        if w[p] == 0 or full.size < 2:
            continue
        assert (np.diff(full) > 0).all() and full[-1] < N, p
        ii, jj = _tril(full.size)
        exp[full[ii] * (full[ii] - 1) // 2 + full[jj]] += dtype(w[p])          # (the pairs of one list are distinct cells)
    return exp


def census(pat, width, N, wrapped=True):
    """What the first-block kernels are given, counted on the host.  A first-block record (X, X, F0, w) is ELIGIBLE when its node has at
    most two blocks, a weight, two ids or more in its full list and two or more of them in its first block X.  n_first: the eligible
    records; n_flat: those with a weight below 128 (the matrix-core step's, kmdb_stats.n_direct in mode 2); per weight 127 / 128 their
    numbers; wrapped: cells whose exact sum is 2^32 or more (None with wrapped=False: the counts alone); last_block: samples in the last block."""
    w = pat["num_kmers"].numpy()
    n_first = n_flat = w127 = w128 = 0
    for p, full in enumerate(full_lists(pat)):
        if w[p] == 0 or full.size < 2:
            continue
        blk = full // width
        if np.unique(blk).size > 2 or int((blk == blk[0]).sum()) < 2:
            continue
        n_first += 1
        n_flat += int(w[p] < 128)
        w127 += int(w[p] == 127)
        w128 += int(w[p] == 128)
    n_wrapped = int((definition(pat, N, dtype=np.uint64) >= (1 << 32)).sum()) if wrapped else None
    return {"n_first": n_first, "n_flat": n_flat, "w127": w127, "w128": w128, "wrapped": n_wrapped,
            "last_block": N - (N - 1) // width * width}


def sparse_rows(exp, N):
    """(row_ptr, col, val) of the non-zeros of a dense lower triangle, as kmdb_all2all_sparse returns them"""
    nz = np.nonzero(exp)[0].astype(np.int64)
    starts = np.arange(N + 1, dtype=np.int64) * (np.arange(N + 1, dtype=np.int64) - 1) // 2          # cell index of (i, 0)
    row = np.searchsorted(starts, nz, side="right") - 1
    row_ptr = np.zeros(N + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(row, minlength=N))
    return row_ptr, nz - starts[row], exp[nz]


def describe_mismatch(got, exp, N):
    bad = np.nonzero(got != exp)[0]
    if bad.size == 0:
        return "equal"
    c = int(bad[0])
    i = int((1 + np.sqrt(1 + 8 * c)) // 2)
    while i * (i - 1) // 2 > c:
        i -= 1
    while (i + 1) * i // 2 <= c:
        i += 1
    return "%d of %d cells differ; first: cell (%d, %d) got %d, expected %d" % (bad.size, exp.size, i, c - i * (i - 1) // 2, int(got[c]), int(exp[c]))


def make_view(K, S, pat, N, tables=None):
    arr = S.to_view_arrays(pat)
    kw = {} if tables is None else {"bucket_offset": tables[0], "slots": tables[1]}
    return arr, K.make_view(18, N, arr["num_kmers"], arr["parent_id"], arr["num_samples"], arr["num_local"], arr["last_sample_id"], arr["num_bits"],
                            arr["data_offset"], arr["data"], **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# child process: the switches read once per process
# ------------------------------------------------------------------------------------------------------------------------------------
def _child(label):
    sys.path.insert(0, ROOT)
    import importlib
    from _kmerdb_loader import import_kmerdb_amd
    from test_gpu_parity import _random_forest
    K = import_kmerdb_amd()
    S = importlib.import_module("kmerdb_amd.synth")
    assert K.device_count() > 0, "needs an MI355X"
    NF = K.capi.FLAG_NO_FALLBACK
    cases = bad = 0

    def check(what, got, exp, N):
        nonlocal cases, bad
        cases += 1
        if not np.array_equal(got, exp):
            bad += 1
            print("MISMATCH %s %s: %s" % (label, what, describe_mismatch(got, exp, N) if got.shape == exp.shape else "shapes differ"), flush=True)

    def run(what, view, exp, N, width):
        d = K.DeviceDB(view, device=0)
        got = d.all2all_dense(flags=NF)
        st = d.stats()
        assert st["path"] == K.capi.PATH_RECORDS and (width is None or st["width"] == width), (what, st)
        check(what + " cold", got, exp, N)
        check(what + " warm", d.all2all_dense(flags=NF), exp, N)
        assert d.stats()["sized_call"] == 0, what
        sp = d.all2all_sparse()
        rp, col, val = sparse_rows(exp, N)
        check(what + " sparse row_ptr", sp.row_ptr, rp, 0)
        check(what + " sparse col", sp.col, col, 0)
        check(what + " sparse val", sp.val, val, 0)
        d.close()

    for width in (50, 64):
        for N in edge_sizes(width):
            pat = edge_forest(width, N)
            exp = definition(pat, N)
            _, view = make_view(K, S, pat, N)
            for nseg in (None, "64"):
                os.environ["KMDB_BLOCK_WIDTH"] = str(width)
                os.environ.pop("KMDB_NSEG", None)
                if nseg:
                    os.environ["KMDB_NSEG"] = nseg
                run("edge forest width %d N %d nseg %s" % (width, N, nseg), view, exp, N, width)
    os.environ.pop("KMDB_NSEG", None)
    N = 1000
    pat = _random_forest(np.random.default_rng(41), N, 6000, 60, heavy_frac=0.4, chain_frac=0.2)
    _, view = make_view(K, S, pat, N)
    os.environ.pop("KMDB_BLOCK_WIDTH", None)
    d = K.DeviceDB(view, device=0)
    exp = d.all2all_dense(flags=K.capi.FLAG_FORCE_GLOBAL_ATOMICS)              # the v1 kernel, itself pinned to the oracle by test_random_forests_bit_exact
    d.close()
    for width in (None, 32):
        if width:
            os.environ["KMDB_BLOCK_WIDTH"] = str(width)
        run("random forest 41 width %s" % width, view, exp, N, width)
    print("%d cases, %d mismatches" % (cases, bad), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1] if len(sys.argv) > 1 else "default"))
